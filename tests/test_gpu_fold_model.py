"""GPU: HPLFlowNet's inference forward with the Up layers' bias-only 1x1 convs folded into their consumers.

The pairs are the small ones of tests/test_gpu_plan.py: N = 300 / 211, N = 40, and the ragged batch of the two.  Folded, the
native plan and the Python pair path issue the same launches on the same folded tensors: bit-identical flows, also after an
in-place update of every parameter and after the parameters were replaced.  The folded flow meets the project's bar against
the float64 torch oracle (2e-4 x max(1, max|flow|), tests/test_gpu_bench_size.py) and is no further from it than twice the
unfolded forward's error (HPL_FOLD_UP=0 in a child process; the two differ only in where roundings fall).  With and without
the slice bias (bcn_use_bias)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from hplflownet_amd.synthetic import SCALES_FILTER_MAP, fill_module_, synthetic_pair

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [(300, 211), (40, 40)]


def make(bias):
    import hplflownet_amd as H
    args = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP, evaluate=True, use_leaky=True,
                                 bcn_use_bias=bias, bcn_use_norm=True, last_relu=False, DEVICE='cuda')
    m = fill_module_(H.HPLFlowNet(args), 1.0, 'hash').to(DEV).eval()
    return m, H.GenerateDataUnsymmetric(args, device=DEV, wide_up=m.lattice_hint())


def clouds():
    out = []
    for b, (n1, n2) in enumerate(COUNTS):
        p1, p2, _ = synthetic_pair(max(n1, n2), 4 + 5 * b)
        out.append((torch.from_numpy(np.ascontiguousarray(p1[:n1].T)).to(DEV), torch.from_numpy(np.ascontiguousarray(p2[:n2].T)).to(DEV)))
    return out


def forwards(m, gen, native):
    """flows of the two pairs alone and of their ragged batch: [(3, N1_b)] * 2 + [(3, N1_b)] * 2, cloned"""
    cl = clouds()
    m.native_forward = native
    try:
        with torch.no_grad():
            out = [m(a[None], b[None], gen.build_native(a, b))[0].clone() for a, b in cl]
            p1, p2 = [a for a, _ in cl], [b for _, b in cl]
            out += [f[0].clone() for f in m(p1, p2, gen.build_native_batch(p1, p2))]
    finally:
        del m.native_forward
    torch.cuda.synchronize()
    return out


def save_flows(path):
    """child-process entry: the native flows of both variants under this process's environment"""
    res = {}
    for bias in (True, False):
        m, gen = make(bias)
        res[bias] = [f.cpu() for f in forwards(m, gen, True)]
    torch.save(res, path)


@pytest.fixture(scope='module')
def unfolded(tmp_path_factory):
    f = str(tmp_path_factory.mktemp('fold') / 'unfolded.pt')
    code = ("import sys\nsys.path.insert(0, %r)\nsys.path.insert(0, %r)\nimport test_gpu_fold_model as T\nT.save_flows(sys.argv[1])\n"
            % (ROOT, os.path.join(ROOT, 'tests')))
    r = subprocess.run([sys.executable, '-c', code, f], cwd=ROOT, env=dict(os.environ, HPL_FOLD_UP='0'), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(f)


def _folding_or_rerun(case):
    """True when this process folds.  Under HPL_FOLD_UP=0 the package of this process cannot: the same case is run by a child
    pytest with the switch on, and must pass there."""
    from hplflownet_amd import ops
    if ops.FOLD_UP:
        return True
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider',
                        os.path.join(ROOT, 'tests', 'test_gpu_fold_model.py') + '::test_folded_forward[%s]' % case],
                       cwd=ROOT, env=dict(os.environ, HPL_FOLD_UP='1'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return False


@pytest.mark.parametrize('bias', [True, False])
def test_folded_forward(bias, unfolded):
    if not _folding_or_rerun(bias):
        return
    from test_gpu_range_guard import oracle_flow
    m, gen = make(bias)
    assert m.fold_up()
    nat, py = forwards(m, gen, True), forwards(m, gen, False)
    plan0 = m.forward_plan()
    assert len(plan0.prog.folds) == 7 and all(o.cond == 0 for o in plan0.prog.ops)
    for a, b in zip(nat, py):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    # against float64, and against the unfolded forward's error on the same pairs (the ragged batch: each pair's own oracle)
    cl = clouds()
    refs = [oracle_flow(m, gen.build_native(a, b), a, b) for a, b in cl]
    for i, f in enumerate(nat):
        ref = refs[i % 2]
        scale = max(1.0, float(ref.abs().max()))
        e_f = float((f.cpu().double() - ref).abs().max())
        e_u = float((unfolded[bias][i].double() - ref).abs().max())
        print('bias=%s %s pair %d (N=%d): max|flow - float64| folded %.3g, unfolded %.3g (bar %.3g)'
              % (bias, 'ragged' if i >= 2 else 'single', i % 2, f.shape[1], e_f, e_u, 2e-4 * scale))
        assert e_f < 2e-4 * scale
        assert e_f <= 2 * e_u
    # what an optimiser step does: the folded weights follow, both paths still agree
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.01)
    nat1, py1 = forwards(m, gen, True), forwards(m, gen, False)
    assert m.forward_plan() is plan0
    for a, b, a0 in zip(nat1, py1, nat):
        assert torch.equal(a, b) and not torch.equal(a, a0)
    # parameters replaced by new tensors: a new plan, new folded tensors, the same flows
    m.float().to('cpu').to(DEV)
    nat2, py2 = forwards(m, gen, True), forwards(m, gen, False)
    assert m.forward_plan() is not plan0
    for a, b, a1 in zip(nat2, py2, nat1):
        assert torch.equal(a, b) and torch.equal(a, a1)
