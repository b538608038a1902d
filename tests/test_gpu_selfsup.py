"""GPU: hpl_selfsup_loss / ops.selfsup_loss, ops.SelfSupLossFn, flownet.selfsup_loss and Trainer(loss='selfsup') (DESIGN.md
§20) against the numpy restatement tests/selfsup_oracle.py.

Bars.  The neighbour assignments are compared exactly: the searches are float32 with one operation order and one tie rule on
both sides.  Each loss component lies within 2 float32 ulps of the restatement's: both add float64 terms, in different orders
(about N 2^-53 relative), and the one rounding to float32 can then land on the neighbouring value.  dflow: rtol 2^-22 plus an
atol of 2^-40 x the pair's largest |dflow| component, for the same reason; the order of the terms is the interface's."""
import numpy as np
import pytest
import torch

from batch64 import counts64, prefix_of
from selfsup_oracle import selfsup

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BLOCK, TILE, SHORT = 256, 1024, 16             # csrc/selfsup_loss.hip: SS_BLOCK, SS_TILE, SS_SHORT


def test_constants_are_the_kernel_s():
    import os
    import re
    from common import ROOT
    src = open(os.path.join(ROOT, 'hplflownet_amd', 'csrc', 'selfsup_loss.hip')).read()
    got = {n: int(re.search(r'constexpr int %s = (\d+);' % n, src).group(1)) for n in ('SS_BLOCK', 'SS_TILE', 'SS_SHORT')}
    assert got == {'SS_BLOCK': BLOCK, 'SS_TILE': TILE, 'SS_SHORT': SHORT}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def cloud(n1, n2, seed, kind='random'):
    """pc1 (3, n1), flow (3, n1), pc2 (3, n2).  'integer': small integer coordinates and flows -- many exact ties and
    duplicated points."""
    rng = np.random.RandomState(seed)
    if kind == 'integer':
        x = rng.randint(0, 4, (3, n1)).astype(np.float32)
        f = rng.randint(-1, 2, (3, n1)).astype(np.float32)
        q = rng.randint(-1, 5, (3, n2)).astype(np.float32)
    else:
        x = rng.uniform(-4, 4, (3, n1)).astype(np.float32)
        f = rng.normal(0, 0.2, (3, n1)).astype(np.float32)
        q = rng.uniform(-4, 4, (3, n2)).astype(np.float32)
        m = min(n1, n2) // 2                     # half of pc2 lies near warped points, and two points are duplicated
        q[:, :m] = (x + f)[:, :m] + rng.normal(0, 0.05, (3, m)).astype(np.float32)
        if n1 > 4:
            x[:, 3] = x[:, 1]
    return x, f, q


def run(x, f, q, k=8, wc=1.0, ws=1.0, p1=None, p2=None, need_grad=True, flow_rows=False):
    from hplflownet_amd import ops
    fl = dev(f.T) if flow_rows else dev(f)
    out = ops.selfsup_loss(dev(x), fl, dev(q), k, wc, ws, p1, p2, need_grad=need_grad, return_neighbors=True)
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all((x is None and y is None) or torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def check(got, o, what, p1=None):
    """got: the op's five outputs; o: the restatement's."""
    loss, dflow, nn12, nn21, nbr = [None if t is None else t.cpu().numpy() for t in got]
    assert np.array_equal(nn12, o['nn12']), what
    assert np.array_equal(nn21, o['nn21']), what
    assert np.array_equal(nbr, o['nbr']), what
    want = o['loss']
    with np.errstate(invalid='ignore'):
        ulps = np.abs(loss.astype(np.float64) - want) / np.spacing(np.abs(want))
    both_nan = np.isnan(loss) & np.isnan(want)
    print('%s: loss %s, worst component %.3g ulps from the restatement' % (what, loss[0], np.nanmax(np.where(both_nan, 0, ulps))))
    assert (both_nan | (ulps <= 2)).all(), (what, loss, want)
    if dflow is None:
        return
    g = o['dflow64']
    N1 = g.shape[0]
    pp = [0, N1] if p1 is None else p1
    worst = 0.0
    for b in range(len(pp) - 1):
        gb, db = g[pp[b]:pp[b + 1]], dflow[pp[b]:pp[b + 1]].astype(np.float64)
        fin = np.isfinite(gb)
        assert np.array_equal(np.isnan(gb), np.isnan(db)), what
        if not fin.any():
            continue
        atol = 2.0 ** -40 * np.abs(gb[fin]).max()
        err = np.abs(db - gb)[fin] - (2.0 ** -22 * np.abs(gb[fin]) + atol)
        worst = max(worst, float((np.abs(db - gb)[fin] / np.maximum(np.abs(gb[fin]), 1e-300)).max()))
        assert (err <= 0).all(), (what, b, float(err.max()))
    print('%s: worst relative |dflow - restatement| %.3g (rtol %.3g)' % (what, worst, 2.0 ** -22))


#: (N1, N2, k): every size of {1, 2, 3, BLOCK-1, BLOCK, BLOCK+1, TILE, TILE+1, 2 TILE+3} on both sides, N1 != N2 both ways
SHAPES = [(1, 2, 1), (2, 1, 3), (3, 2, 8), (2, 3, 8), (3, 3, 3),
          (BLOCK - 1, BLOCK + 1, 3), (BLOCK, BLOCK - 1, 8), (BLOCK + 1, BLOCK, 1), (BLOCK - 1, 3, 8), (1, BLOCK, 1),
          (TILE, TILE + 1, 8), (TILE + 1, TILE, 3), (2 * TILE + 3, TILE, 1), (TILE, 2 * TILE + 3, 8), (2 * TILE + 3, 2 * TILE + 3, 3),
          (BLOCK + 1, 2 * TILE + 3, 1), (2 * TILE + 3, BLOCK - 1, 8)]


@pytest.mark.parametrize('n1,n2,k', SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('kind', ['random', 'integer'])
def test_against_the_restatement(n1, n2, k, kind):
    x, f, q = cloud(n1, n2, 1000 * n1 + n2 + k, kind)
    o = selfsup(x, f, q, k, 0.75, 1.5)
    check(run(x, f, q, k, 0.75, 1.5), o, '%s N1 = %d N2 = %d k = %d' % (kind, n1, n2, k))


def test_flow_strides_and_padded_rows_give_the_same_bits():
    from hplflownet_amd import ops
    n1, n2, k = BLOCK + 1, TILE + 1, 3
    x, f, q = cloud(n1, n2, 5)
    base = run(x, f, q, k)
    assert same(base, run(x, f, q, k, flow_rows=True))       # the forward's point-major [N][3] rows
    wide = torch.full((n1, 7), float('nan'), device=DEV)     # rows of a wider buffer, poisoned around the flow
    wide[:, 2:5] = dev(f.T)
    wide_t = torch.full((3, n1 + 9), float('nan'), device=DEV)
    wide_t[:, 4:4 + n1] = dev(f)
    pad1 = torch.full((3, n1 + 5), float('nan'), device=DEV)
    pad1[:, 2:2 + n1] = dev(x)
    pad2 = torch.full((3, n2 + 11), float('nan'), device=DEV)
    pad2[:, 7:7 + n2] = dev(q)
    for fl in (wide[:, 2:5], wide_t[:, 4:4 + n1]):
        got = ops.selfsup_loss(pad1[:, 2:2 + n1], fl, pad2[:, 7:7 + n2], k, return_neighbors=True)
        assert pad1[:, 2:2 + n1].stride(0) == n1 + 5
        assert same(base, got)
    check(base, selfsup(x, f, q, k), 'strided')


def test_skewed_chamfer_list():
    """All N2 = TILE + 1 points of pc2 are nearest ONE warped point: its incoming list is the whole cloud."""
    n1, n2 = BLOCK + 44, TILE + 1
    rng = np.random.RandomState(7)
    g = np.stack(np.meshgrid(np.arange(10.0), np.arange(6.0), np.arange(5.0), indexing='ij')).reshape(3, -1) * 10
    x = (g + rng.uniform(-1, 1, g.shape)).astype(np.float32)
    f = rng.normal(0, 0.3, x.shape).astype(np.float32)
    q = ((x + f)[:, 77:78] + rng.normal(0, 0.05, (3, n2))).astype(np.float32)
    assert x.shape[1] == n1
    o = selfsup(x, f, q, 3)
    assert (o['nn21'] == 77).all()
    check(run(x, f, q, 3), o, 'skew')


@pytest.mark.parametrize('n,k', [(SHORT + 1, 1), (SHORT + 2, 1), (BLOCK + 44, 1), (BLOCK + 44, 3), (4 * 64 + 1 + 3, 3)])
def test_star_graph(n, k):
    """Every point of pc1 at ONE position: all d2 tie at 0 and go to the smallest indices, so points 0 .. k-1 are listed by
    all others (in-degree n - 1, around SS_SHORT and over several 64-entry rounds)."""
    rng = np.random.RandomState(n + k)
    x = np.repeat(np.array([[1.0], [2.0], [3.0]], np.float32), n, axis=1)
    f = rng.normal(0, 0.5, (3, n)).astype(np.float32)
    q = rng.uniform(-2, 5, (3, 5)).astype(np.float32)
    o = selfsup(x, f, q, k)
    assert (o['nbr'][0, 1:] == 0).all() and (o['nbr'] == 0).sum() == n - 1
    check(run(x, f, q, k), o, 'star n = %d k = %d' % (n, k))


def test_without_gradient_and_without_graph():
    x, f, q = cloud(BLOCK + 1, TILE + 1, 11)
    full = run(x, f, q, 3)
    lean = run(x, f, q, 3, need_grad=False)
    assert lean[1] is None and same((full[0],) + full[2:], (lean[0],) + lean[2:])
    o = selfsup(x, f, q, 0, 1.25, 0.0)
    got = run(x, f, q, 0, 1.25, 0.0)
    assert got[4].shape == (0, BLOCK + 1)
    check(got, o, 'k = 0')
    assert float(got[0][0, 3]) == 0.0
    assert same(got[:4], run(x, f, q, 0, 1.25, 0.0)[:4])     # (and a second call gives the same bits)


def test_zero_flow_on_the_same_cloud():
    x, _, _ = cloud(TILE + 1, TILE + 1, 13)
    loss, dflow, nn12, nn21, _ = run(x, np.zeros_like(x), x, 3)
    assert float(loss[0, 1]) == 0.0 and float(loss[0, 2]) == 0.0 and float(loss[0, 3]) == 0.0 and float(loss[0, 0]) == 0.0
    assert not dflow.any()
    # (a duplicated point takes the smaller index of the two)
    want = np.arange(TILE + 1)
    want[3] = 1
    assert np.array_equal(nn12.cpu().numpy(), want) and np.array_equal(nn21.cpu().numpy(), want)


# ----------------------------------------------------------------------------- batches
PAIRS = [(BLOCK + 44, BLOCK + 1), (0, 0), (130, 0), (2, 3)]


def batch_of(order, seed=21):
    xs, fs, qs = zip(*[cloud(PAIRS[i][0], PAIRS[i][1], seed + i) for i in order])
    p1, p2 = [0], [0]
    for i in order:
        p1.append(p1[-1] + PAIRS[i][0])
        p2.append(p2[-1] + PAIRS[i][1])
    return np.concatenate(xs, 1), np.concatenate(fs, 1), np.concatenate(qs, 1), p1, p2


def piece(res, pp1, pp2, b):
    """Pair b's outputs of a batch, its indices relative to the pair's first points."""
    loss, dflow, nn12, nn21, nbr = res
    s1, s2 = slice(pp1[b], pp1[b + 1]), slice(pp2[b], pp2[b + 1])
    rel = lambda t, off: torch.where(t >= 0, t - off, t)          # noqa: E731
    return (loss[b], dflow[s1], rel(nn12[s1], pp2[b]), rel(nn21[s2], pp1[b]), rel(nbr[:, s1], pp1[b]))


def test_ragged_batch_against_the_restatement_and_bit_stable():
    """B = 4 ragged: an empty pair in the middle, a pair with N2 = 0, a pair of 2 points with k = 8.  Every pair's outputs are
    the same bits alone and in a batch of another order."""
    k = 8
    order = [0, 1, 2, 3]
    x, f, q, p1, p2 = batch_of(order)
    got = run(x, f, q, k, 0.75, 1.5, p1, p2)
    check(got, selfsup(x, f, q, k, 0.75, 1.5, p1, p2), 'ragged B = 4', p1)
    assert not got[0][1].any()                               # the empty pair
    assert float(got[0][2, 1]) == 0.0 and float(got[0][2, 2]) == 0.0 and float(got[0][2, 3]) > 0
    other = [3, 2, 0, 1]
    xo, fo, qo, o1, o2 = batch_of(other)
    goto = run(xo, fo, qo, k, 0.75, 1.5, o1, o2)

    for b, i in enumerate(order):
        xa, fa, qa = cloud(PAIRS[i][0], PAIRS[i][1], 21 + i)
        alone = run(xa, fa, qa, k, 0.75, 1.5)
        assert same(piece(got, p1, p2, b), piece(alone, [0, PAIRS[i][0]], [0, PAIRS[i][1]], 0)), i
        assert same(piece(got, p1, p2, b), piece(goto, o1, o2, other.index(i))), i


def test_a_batch_of_64_pairs_equals_its_pairs():
    """B = 64 (tests/batch64.py; pc2's sizes differ from pc1's, one pair has no pc2, and the two pairs of several workgroups
    swap their sizes): the restatement's outputs, and every pair's are the bits of that pair run alone with its own prefixes."""
    k = 8
    n1 = counts64()
    n2 = [0 if n == 0 else 1 + (11 * i) % 300 for i, n in enumerate(n1)]
    n2[3], n2[40], n2[50] = 0, n1[50], n1[40]
    clouds = [cloud(a, b, 640 + i) for i, (a, b) in enumerate(zip(n1, n2))]
    x, f, q = (np.concatenate([c[j] for c in clouds], 1) for j in range(3))
    p1, p2 = prefix_of(n1), prefix_of(n2)
    got = run(x, f, q, k, 0.75, 1.5, p1, p2)
    check(got, selfsup(x, f, q, k, 0.75, 1.5, p1, p2), 'B = 64', p1)
    for b, (xa, fa, qa) in enumerate(clouds):
        alone = run(xa, fa, qa, k, 0.75, 1.5, [0, n1[b]], [0, n2[b]])
        assert same(piece(got, p1, p2, b), piece(alone, [0, n1[b]], [0, n2[b]], 0)), b


# ----------------------------------------------------------------------------- non-finite inputs
def test_a_nan_point_is_nobody_s_nearest_point():
    n1, n2, k = BLOCK + 1, BLOCK - 1, 3
    x, f, q = cloud(n1, n2, 31)
    q[1, 5] = np.nan
    f[0, 9] = np.nan
    o = selfsup(x, f, q, k, 0.75, 1.5)
    got = run(x, f, q, k, 0.75, 1.5)
    loss, dflow, nn12, nn21, nbr = [t.cpu().numpy() for t in got]
    assert (nn12 != 5).all() and (nn21 != 9).all() and nn21[5] == -1 and nn12[9] == -1
    check(got, o, 'NaN')                                     # (index sets, NaN pattern and every finite value)
    assert np.isfinite(loss[0, 1:3]).all() and np.isnan(loss[0, 3])      # the graph is over positions: the flow's NaN is in S
    listing = (o['nbr'] == 9).any(0)
    listing[9] = True
    listing |= (o['nbr'][:, 9][:, None] == np.arange(n1)[None, :]).any(0)     # (and the points point 9 lists)
    # (the sums are per component: the NaN of flow component 0 stays in component 0 of the gradients it reaches)
    assert np.isfinite(dflow[~listing]).all() and np.isnan(dflow[9, 0]) and np.isfinite(dflow[9, 1:]).all()
    assert np.isnan(dflow[listing][:, 0]).all() and np.isfinite(dflow[listing][:, 1:]).all()
    # with the Chamfer terms alone the NaN points add 0 and every other output is finite
    o0 = selfsup(x, f, q, 0, 1.0, 0.0)
    got0 = run(x, f, q, 0, 1.0, 0.0)
    check(got0, o0, 'NaN, Chamfer alone')
    assert np.isfinite(got0[0].cpu().numpy()).all() and np.isfinite(np.delete(got0[1].cpu().numpy(), 9, 0)).all()


# ----------------------------------------------------------------------------- autograd
def test_autograd_hands_back_the_op_s_gradient():
    """B = 4 (a power of two: the mean's 1 / B scales exactly).  flow.grad is ops.selfsup_loss's dflow / B bit for bit; an
    upstream factor of 2 doubles it exactly."""
    from hplflownet_amd import flownet, ops
    B, n1, n2, k = 4, BLOCK + 1, BLOCK - 1, 3
    xs, fs, qs = zip(*[cloud(n1, n2, 41 + b) for b in range(B)])
    pc1, pc2 = dev(np.stack(xs)), dev(np.stack(qs))
    flow = dev(np.stack(fs)).requires_grad_(True)            # (B, 3, N): the form of the models' batched output
    L, comps = flownet.selfsup_loss(flow, pc1, pc2, k=k, w_chamfer=0.75, w_smooth=1.5)
    L.backward()
    p1, p2 = [n1 * b for b in range(B + 1)], [n2 * b for b in range(B + 1)]
    loss, dflow = ops.selfsup_loss(dev(np.concatenate(xs, 1)), dev(np.concatenate(fs, 1)), dev(np.concatenate(qs, 1)), k, 0.75, 1.5,
                                   p1, p2)
    assert torch.equal(bits(comps), bits(loss)) and not comps.requires_grad
    assert torch.equal(bits(L.detach()), bits(loss[:, 0].mean()))
    want = (dflow / B).view(B, n1, 3).transpose(1, 2)
    assert torch.equal(bits(flow.grad), bits(want))
    assert pc1.grad is None and pc2.grad is None
    g1 = flow.grad.clone()
    flow.grad = None
    (2 * flownet.selfsup_loss(flow, pc1, pc2, k=k, w_chamfer=0.75, w_smooth=1.5)[0]).backward()
    assert torch.equal(bits(flow.grad), bits(2 * g1))
    # the other forms: one (3, N) pair with a [N, 3] leaf behind it, and lists of a ragged batch
    rows = dev(fs[0].T).requires_grad_(True)
    flownet.selfsup_loss(rows.t(), dev(xs[0]), dev(qs[0]), k=k)[0].backward()
    assert torch.equal(bits(rows.grad), bits(ops.selfsup_loss(dev(xs[0]), dev(fs[0]), dev(qs[0]), k)[1]))
    x2, f2, q2 = cloud(37, 50, 47)
    leaves = [dev(fs[0]).requires_grad_(True), dev(f2)[None].requires_grad_(True)]
    Lr, cr = flownet.selfsup_loss(leaves, [dev(xs[0]), dev(x2)[None]], [dev(qs[0]), dev(q2)[None]], k=k)
    Lr.backward()
    _, d = ops.selfsup_loss(dev(np.concatenate([xs[0], x2], 1)), dev(np.concatenate([fs[0], f2], 1)),
                            dev(np.concatenate([qs[0], q2], 1)), k, prefix1=[0, n1, n1 + 37], prefix2=[0, n2, n2 + 50])
    assert torch.equal(bits(leaves[0].grad), bits((d[:n1] / 2).t())) and torch.equal(bits(leaves[1].grad[0]), bits((d[n1:] / 2).t()))
    assert tuple(cr.shape) == (2, 4)


# ----------------------------------------------------------------------------- whole model
def _pair(n=256, seed=0):
    from hplflownet_amd.synthetic import synthetic_pair
    pc1, pc2, sf = synthetic_pair(n, seed)
    return dev(pc1.T), dev(pc2.T), torch.full((3, n), float('nan'), device=DEV), dev(sf.T)


def _params(tr):
    return [p.detach().clone() for p in tr.model.parameters()]


def test_trainer_step_is_the_hand_written_step():
    from hplflownet_amd import engine, ops
    pc1, pc2, nan_sf, sf = _pair()
    tr = engine.Trainer('HPLFlowNetShallow', DEV, init='hash', loss='selfsup')
    assert not tr.native_step
    before = _params(tr)
    loss = tr.train_step(pc1, pc2, nan_sf, tr._single_lattice(pc1, pc2))
    after = _params(tr)
    assert torch.isfinite(loss) and all(torch.isfinite(p).all() for p in after) and tr.native_steps == 0
    sup = engine.Trainer('HPLFlowNetShallow', DEV, init='hash', loss='epe3d', native_step=False)
    sup_before = _params(sup)
    sup.train_step(pc1, pc2, sf, sup._single_lattice(pc1, pc2))
    moved = 0
    for b, a, sb, sa in zip(before, after, sup_before, _params(sup)):
        if not torch.equal(sb, sa):
            moved += 1
            assert not torch.equal(b, a)
    assert moved > 0

    def by_hand():
        h = engine.Trainer('HPLFlowNetShallow', DEV, init='hash', native_step=False)
        flow = h.model(pc1[None], pc2[None], h._single_lattice(pc1, pc2))
        _, dflow = ops.selfsup_loss(pc1, flow.detach()[0], pc2, 8, 1.0, 1.0)
        h.opt.zero_grad(set_to_none=True)
        flow.backward(dflow.t()[None])
        h.opt.step()
        return _params(h)

    def by_trainer():
        t = engine.Trainer('HPLFlowNetShallow', DEV, init='hash', loss='selfsup')
        t.train_step(pc1, pc2, nan_sf, t._single_lattice(pc1, pc2))
        return _params(t)

    def apart(x, y):
        return max(float((a - b).abs().max()) for a, b in zip(x, y))
    # The backward's scatter kernels add with atomics: two runs of ONE program need not agree in the last bits, and Adam's first
    # step (lr * g / (|g| + eps)) turns a last-bit change of a gradient near eps into a visible change of its parameter, so a run
    # falls into one of a few modes.  Measured on an MI355X over 8 hand-written and 4 trainer steps: hand-written pairs 1.7e-08
    # to 4.2e-07 apart, trainer against hand-written 1.5e-08 to 7.6e-07, both in clusters (2e-08 .. 7e-08 and 3.4e-07 .. 7.6e-07).
    # One sample of the spread against one sample of the distance is therefore a coin: 4 runs of each give 6 samples of the
    # spread, and the trainer's step is the hand-written one when SOME run of it is within that spread of SOME hand-written run (a
    # step that computes something else is lr-sized, 1e-4, away from every one of them).
    hands = [by_hand() for _ in range(4)]
    trained = [after] + [by_trainer() for _ in range(3)]
    spread = max(apart(hands[i], hands[j]) for i in range(4) for j in range(i))
    diff = min(apart(t, h) for t in trained for h in hands)
    print('hand-written steps: up to %.3g apart; the trainer\'s nearest to one of them: %.3g' % (spread, diff))
    if spread == 0.0:
        assert diff == 0.0
    else:
        assert diff <= 2 * spread


def test_trainer_batched_steps():
    from hplflownet_amd import engine
    a, b = _pair(256, 0), _pair(256, 1)
    p1, p2, nan_sf = torch.stack([a[0], b[0]]), torch.stack([a[1], b[1]]), torch.stack([a[2], b[2]])
    tr = engine.Trainer('HPLFlowNetShallow', DEV, init='hash', loss='selfsup', selfsup={'k': 4, 'w_smooth': 0.5})
    lat = tr.gen.build_native_batch(p1, p2, for_training=True)
    for _ in range(3):
        losses = tr.train_step_batch(p1, p2, nan_sf, lat)
        assert tuple(losses.shape) == (2,) and torch.isfinite(losses).all()
    assert tr.native_steps == 0 and all(torch.isfinite(p).all() for p in tr.model.parameters())


def test_engine_trains_with_the_selfsup_loss():
    from hplflownet_amd import engine
    engine.main(['--loss', 'selfsup', '--arch', 'HPLFlowNetShallow', '--points', '256', '--pairs', '2', '--epochs', '1'])
