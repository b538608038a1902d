"""GPU: whole forwards whose activations take the range guard's second pass (csrc/gconv3.hip GUARD launches).

The pair below is two parts 100 units apart -- far more than the coarsest lattice cell, so that no vertex, blur neighbour or
correlation tap mixes them at any level: a frustum of 7 168 points (|p| up to ~135) and 1 024 points within 1e-7 of the origin,
cloud 2's moved by as little.  With every bias of the model zeroed, LeakyReLU and the normalised splat are positively
homogeneous, and conv1's first weight carries a gain of 1e7: every activation row of the quiet part sits ~2^33 below the loud
part's rows of the same matrix -- inside the 2^41 the second pass covers, and far enough for the unguarded pair form to lose
the quiet rows' low bits.  The flow is compared, point by point relative to the largest flow of the point's own part, with the
float64 torch oracle (oracle/torch_oracle.py) on the same lattice, and with the same forward under HPL_MATH=f32 (the fp32-MFMA
kernels) and HPL_RANGE_GUARD=0 (the pair form without its guard) in child processes."""
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
N, NQ = 8192, 1024            # points per cloud, of which the last NQ are the quiet part
GAIN, SHIFT = 1e7, 100.0


def _skip_unless_pairs():
    from hplflownet_amd import ops
    if ops.SPLIT_PLANES != 2 or not ops.SPLIT3:
        pytest.skip('the range guard belongs to the fp16-pair form (HPL_MATH=f16x2, the default)')


def loud_and_quiet_pair(seed=0):
    """(pc1, pc2) float32 (N, 3): the frustum of synthetic_pair moved SHIFT along z, then NQ points inside |p| < 1e-7"""
    a, c, _ = synthetic_pair(N - NQ, seed)
    rng = np.random.RandomState(seed + 1)
    q1 = rng.uniform(-5e-8, 5e-8, (NQ, 3))
    q2 = q1 + rng.uniform(-2e-8, 2e-8, (NQ, 3))
    shift = np.float32([0.0, 0.0, SHIFT])
    return np.concatenate([a + shift, q1]).astype(np.float32), np.concatenate([c + shift, q2]).astype(np.float32)


def make_model(loud_quiet=True):
    import hplflownet_amd as H
    args = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP, evaluate=True, use_leaky=True,
                                 bcn_use_bias=True, bcn_use_norm=True, last_relu=False, DEVICE='cuda')
    m = fill_module_(H.HPLFlowNet(args), 1.0, 'hash')
    if loud_quiet:
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name.endswith('bias'):
                    p.zero_()
            m.conv1[0].composed_module[0].weight.mul_(GAIN)
    m = m.to(DEV).eval()
    return m, H.GenerateDataUnsymmetric(args, device=DEV, wide_up=m.lattice_hint())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV)


def pairs():
    """the constructed pair and the standard bench pair, as (3, N) device tensors"""
    lq = loud_and_quiet_pair()
    std = synthetic_pair(N, 0)[:2]
    return [(_dev(lq[0]), _dev(lq[1])), (_dev(std[0]), _dev(std[1]))]


def native_flows(m, gen):
    """-> {'single': flow (3, N) of the constructed pair, 'batch': flows (2, 3, N) of the batch [constructed, standard],
    'trips_single' / 'trips_batch': second passes the plan took in each}"""
    (a1, a2), (b1, b2) = pairs()
    plan = m.forward_plan()
    out = {}
    with torch.no_grad():
        lat = gen.build_native(a1, a2)
        t0 = plan.guard_trips()
        out['single'] = m(a1[None], a2[None], lat)[0]
        t1 = plan.guard_trips()
        latb = gen.build_native_batch(torch.stack([a1, b1]), torch.stack([a2, b2]))
        out['batch'] = m(torch.stack([a1, b1]), torch.stack([a2, b2]), latb)
        t2 = plan.guard_trips()
    out['trips_single'], out['trips_batch'] = t1 - t0, t2 - t1
    return out


def save_flows(path):
    """child-process entry: the native flows of the constructed model under this process's environment"""
    m, gen = make_model()
    f = native_flows(m, gen)
    torch.save({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in f.items()}, path)


def oracle_flow(m, lat, p1, p2):
    """float64 torch oracle of the model on the lattice `lat` (one pair) -> (3, N) float64 on the host"""
    import hplflownet_amd as H
    from oracle import torch_oracle as TO
    gd = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()} for d in H.to_reference_format(lat)]
    sd = TO.parameters({k: v.cpu() for k, v in m.state_dict().items()}, requires_grad=False)
    with torch.no_grad():
        return TO.hplflownet_forward(sd, p1.cpu().double(), p2.cpu().double(), TO.lattice(gd))


def part_errors(flow, ref, parts):
    """largest error over the points of each part (max over the 3 components), relative to the part's largest |flow|"""
    d = (flow.cpu().double() - ref).abs().max(dim=0).values
    mag = ref.abs().max(dim=0).values
    return [float(d[sl].max() / mag[sl].max()) for sl in parts]


LQ_PARTS = (slice(0, N - NQ), slice(N - NQ, N))          # loud, quiet
# The quiet part's bar against the f32 forward.  Its rows reach the wide launches ~2^33 below the loud ones: the first split
# leaves their elements' low bits to the second pass, which carries >= 21 bits of every element where an fp32
# operand carries 24 -- over the ~20 wide launches of the forward that is several times the f32 forward's error (measured on
# one MI355X: 2.3e-5 against 4.0e-6 of the part's largest flow, 5.8 x; the loud part: 2.8e-6 against 3.0e-6; the unguarded
# pair form: 0.11).  20 x leaves a 3 x margin and stays 250 x below the unguarded form.
QUIET_VS_F32 = 20
STD_PARTS = (slice(0, N),)


def _child(env, tmp_path, tag):
    f = str(tmp_path / ('%s.pt' % tag))
    code = ("import sys\nsys.path.insert(0, %r)\nsys.path.insert(0, %r)\nimport test_gpu_range_guard as T\nT.save_flows(sys.argv[1])\n"
            % (ROOT, os.path.join(ROOT, 'tests')))
    r = subprocess.run([sys.executable, '-c', code, f], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(f)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """the guarded forwards of this process, the float64 references and the two child runs (f32, unguarded), once"""
    _skip_unless_pairs()
    tmp = tmp_path_factory.mktemp('range_guard')
    m, gen = make_model()
    out = native_flows(m, gen)
    (a1, a2), (b1, b2) = pairs()
    with torch.no_grad():
        lat = gen.build_native(a1, a2)
        m.native_forward = False                   # the Python no-grad pair path (gconv_raw, guarded) on the same lattice
        try:
            out['python'] = m(a1[None], a2[None], lat)[0]
        finally:
            del m.native_forward
    out['ref'] = oracle_flow(m, lat, a1, a2)
    out['ref_std'] = oracle_flow(m, gen.build_native(b1, b2), b1, b2)
    torch.cuda.synchronize()
    out['f32'] = _child({'HPL_MATH': 'f32'}, tmp, 'f32')
    out['off'] = _child({'HPL_RANGE_GUARD': '0'}, tmp, 'off')
    return out


def test_the_bench_pair_takes_no_second_pass():
    """The standard pair of bench.py with the standard model: no launch of its forward trips the guard (bench.py reports
    exact_fallback_launches: 0)."""
    _skip_unless_pairs()
    m, gen = make_model(loud_quiet=False)
    p1, p2 = pairs()[1]
    plan = m.forward_plan()
    with torch.no_grad():
        lat = gen.build_native(p1, p2)
        t0 = plan.guard_trips()
        m(p1[None], p2[None], lat)
        assert plan.guard_trips() == t0


def test_a_forward_that_trips_the_guard_keeps_the_quiet_part_fp32_class(runs):
    """The constructed pair through the native plan: the guard trips, and the quiet part's flow is as close to float64 as the
    fp32-MFMA forward's, where the unguarded pair form is far off; the Python pair path meets the same bar."""
    ref = runs['ref']
    e = part_errors(runs['single'], ref, LQ_PARTS)
    e32 = part_errors(runs['f32']['single'], ref, LQ_PARTS)
    eoff = part_errors(runs['off']['single'], ref, LQ_PARTS)
    epy = part_errors(runs['python'], ref, LQ_PARTS)
    print('second passes: guarded %d, f32 %d, unguarded %d' % (runs['trips_single'], runs['f32']['trips_single'], runs['off']['trips_single']))
    print('flow error / part max (loud, quiet): guarded %.3g %.3g, python %.3g %.3g, f32 %.3g %.3g, unguarded %.3g %.3g'
          % tuple(e + epy + e32 + eoff))
    assert runs['trips_single'] >= 1
    assert runs['f32']['trips_single'] == 0 and runs['off']['trips_single'] == 0
    for got in (e, epy):
        assert got[0] <= 4 * e32[0] + 1e-6
        assert got[1] <= QUIET_VS_F32 * e32[1]
    assert eoff[1] >= 100 * e[1]


def test_a_batch_where_one_pair_makes_the_other_quiet(runs):
    """The batch [constructed pair, standard pair] in one forward: it trips, and each pair's flow meets the same per-part bar
    against its own float64 reference."""
    b, b32, boff = runs['batch'], runs['f32']['batch'], runs['off']['batch']
    print('batch second passes: %d' % runs['trips_batch'])
    assert runs['trips_batch'] >= 1
    for i, (ref, parts) in enumerate(((runs['ref'], LQ_PARTS), (runs['ref_std'], STD_PARTS))):
        e, e32, eoff = [part_errors(x[i], ref, parts) for x in (b, b32, boff)]
        print('batch pair %d: flow error / part max: guarded %s, f32 %s, unguarded %s'
              % (i, ' '.join('%.3g' % x for x in e), ' '.join('%.3g' % x for x in e32), ' '.join('%.3g' % x for x in eoff)))
        assert e[0] <= 4 * e32[0] + 1e-6
        if len(e) > 1:
            assert e[1] <= QUIET_VS_F32 * e32[1]
    assert part_errors(boff[0], runs['ref'], LQ_PARTS)[1] >= 100 * part_errors(b[0], runs['ref'], LQ_PARTS)[1]
