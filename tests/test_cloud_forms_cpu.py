"""The form parsers of flownet on host tensors -- they touch no device --, against a plain restatement: the views
equal the inputs' slices, the prefix equals the cumulative sum, a result goes back into the operand's form."""
import types

import numpy as np
import pytest
import torch

from hplflownet_amd import _lib, flownet as F

SIZES = {1: [7], 3: [7, 4, 9]}                  # unequal N_b


def clouds_of(counts, seed=0, rows=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(rows, n, generator=g) for n in counts]


def same_memory(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


def test_prefix_of_is_the_cumulative_sum():
    assert F._prefix_of([]) == [0] and F._prefix_of([5]) == [0, 5]
    for counts in ([7, 4, 9], [0, 3, 0, 0, 2], range(1, 70)):
        assert F._prefix_of(counts) == [0] + np.cumsum(list(counts)).tolist()
    assert F._prefix_of(torch.Size([3, 4])) == [0, 3, 7] and all(type(x) is int for x in F._prefix_of(torch.Size([3, 4])))
    assert F._prefix_of(c.shape[1] for c in clouds_of([2, 5])) == [0, 2, 7]             # (a generator does)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('rows3', [False, True])
def test_every_form_in(B, rows3):
    cl = clouds_of(SIZES[B])
    # a list, entries (3, N_b) and (1, 3, N_b) mixed
    listed = [c[None] if b % 2 == 0 else c for b, c in enumerate(cl)]
    for seq in (listed, tuple(listed)):
        views, form = F._cloud_forms(seq, 'op', 'pc', rows3)
        assert form == [b % 2 == 0 for b in range(B)] and all(same_memory(v, c) for v, c in zip(views, cl))
        packed = F._packed(seq, views, form)
        assert torch.equal(packed, torch.cat(cl, 1)) and (B > 1 or same_memory(packed, cl[0]))
    # a (B, 3, N) tensor
    x = torch.stack(clouds_of([6] * B))
    views, form = F._cloud_forms(x, 'op', 'pc', rows3)
    assert form is None and len(views) == B and all(same_memory(v, x[b]) for b, v in enumerate(views))
    packed = F._packed(x, views, form)
    assert torch.equal(packed, torch.cat([x[b] for b in range(B)], 1)) and (B > 1 or same_memory(packed, x[0]))
    # a (3, N) tensor: one cloud, or a packed one
    y = torch.cat(cl, 1)
    views, form = F._cloud_forms(y, 'op', 'pc', rows3)
    assert form is False and len(views) == 1 and views[0] is y and F._packed(y, views, form) is y


@pytest.mark.parametrize('B', [1, 3])
def test_every_form_out(B):
    counts = SIZES[B]
    prefix = F._prefix_of(counts)
    rows = torch.arange(3.0 * prefix[-1]).reshape(prefix[-1], 3)                        # a per-point result, [sum N_b, 3]
    got = F._rows_as(rows, [b % 2 == 1 for b in range(B)], prefix)
    assert [tuple(g.shape) for g in got] == [(1, 3, n) if b % 2 else (3, n) for b, n in enumerate(counts)]
    assert all(torch.equal(g.reshape(3, -1), rows[prefix[b]:prefix[b + 1]].t()) and g.data_ptr() == rows[prefix[b]:].data_ptr()
               for b, g in enumerate(got))
    flat = F._rows_as(rows, False, prefix)
    assert flat.shape == (3, prefix[-1]) and torch.equal(flat, rows.t()) and flat.data_ptr() == rows.data_ptr()
    eq = torch.arange(3.0 * 5 * B).reshape(5 * B, 3)
    back = F._rows_as(eq, None, F._prefix_of([5] * B))
    assert back.shape == (B, 3, 5) and all(torch.equal(back[b], eq[5 * b:5 * b + 5].t()) for b in range(B))
    assert back.data_ptr() == eq.data_ptr()


def test_cloud_forms_refusals():
    a = torch.zeros(3, 5)
    tensor_text = 'op: pc is a (3, N) or (B, 3, N) tensor or a list of (3, N_b) tensors'
    list_text = 'op: pc is a tensor or a non-empty list of (3, N_b) tensors'
    for bad in (None, 'x', torch.zeros(5), torch.zeros(1, 1, 3, 5)):
        for rows3 in (False, True):
            with pytest.raises(_lib.HplError) as e:
                F._cloud_forms(bad, 'op', 'pc', rows3)
            assert str(e.value) == tensor_text
    for bad in ([], [None], [a, 'x'], [torch.zeros(5)], [torch.zeros(1, 1, 3, 5)], (a, None)):
        for rows3 in (False, True):
            with pytest.raises(_lib.HplError) as e:
                F._cloud_forms(bad, 'op', 'pc', rows3)
            assert str(e.value) == (tensor_text if rows3 else list_text)
    # 3 rows a cloud, and a cloud at all, are asked for only where the clouds are laid side by side before an op sees them
    for bad in (torch.zeros(5, 3), torch.zeros(2, 4, 5), [a, torch.zeros(2, 5)], torch.zeros(0, 3, 5)):
        with pytest.raises(_lib.HplError) as e:
            F._cloud_forms(bad, 'op', 'pc', True)
        assert str(e.value) == tensor_text
        F._cloud_forms(bad, 'op', 'pc')


def lattice(point_counts=None, batch=None):
    if point_counts is not None:
        return types.SimpleNamespace(ragged=True, point_counts=point_counts, levels=[], batch=len(point_counts))
    return types.SimpleNamespace(ragged=False, levels=[], batch=batch)


def test_counts_from_a_lattice_or_a_sequence():
    rag = lattice([(7, 6), (4, 5), (9, 9)])
    assert F._stated_counts(None, 20) is None and F._pair_counts(None, 20) == [20]
    assert F._pair_counts(rag, 20) == [7, 4, 9] and F._pair_counts(rag, 20, 'op', 0) == [7, 4, 9]
    assert F._pair_counts(rag, 20, 'op', 1) == [6, 5, 9]
    assert F._pair_counts(lattice(batch=4), 20) == [5] * 4 and F._stated_counts(lattice(batch=4)) is None
    assert F._pair_counts(lattice(batch=None), 20) == [20]
    assert F._pair_counts([7, 4, 9], 20) == [7, 4, 9] and F._pair_counts((np.int64(20),), 20) == [20]
    both = ([7, 4, 9], (6, 5, 9))
    assert F._pair_counts(both, 20, 'op', 0) == [7, 4, 9] and F._pair_counts(both, 20, 'op', 1) == [6, 5, 9]
    assert F._pair_counts([[20], [20]][0], 20) == [20]
    for bad, total, kw, text in (([7, 4], 20, {}, 'rigid_refine: the point counts [7, 4] do not add up to 20 points'),
                                 ([21, -1], 20, {}, 'rigid_refine: the point counts [21, -1] do not add up to 20 points'),
                                 (rag, 21, dict(who='op'), 'op: the point counts [7, 4, 9] do not add up to 21 points'),
                                 (lattice(batch=3), 20, dict(who='op'), 'op: the point counts [6, 6, 6] do not add up to 20 points'),
                                 (both, 21, dict(who='op', cloud=1, what=' of pc2'),
                                  'op: the point counts [6, 5, 9] of pc2 do not add up to 21 points')):
        with pytest.raises(_lib.HplError) as e:
            F._pair_counts(bad, total, **kw)
        assert str(e.value) == text


def riders(p):
    return F._pairs_packed(p)[1]


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('corr', [True, False])
@pytest.mark.parametrize('with_pc2', [True, False])
@pytest.mark.parametrize('with_sf', [True, False])
def test_pair_forms_prologue_and_epilogue(B, corr, with_pc2, with_sf):
    n1 = SIZES[B]
    n2 = n1 if corr else [n + 2 for n in n1]
    c1, c2, fl = clouds_of(n1, 1), clouds_of(n2, 2), clouds_of(n1, 3)
    p = F._pairs_in('op', [c[None] for c in c1], c2 if with_pc2 else None, fl if with_sf else None, corr)
    joint = corr or not with_pc2
    want = c1 if joint else c1 + c2
    assert p.joint == joint and len(p.clouds) == len(want) and all(same_memory(a, b) for a, b in zip(p.clouds, want))
    assert p.prefix == [0] + np.cumsum([c.shape[1] for c in want]).tolist()
    assert (p.c2 is None) == (not with_pc2) and (p.fl is None) == (not with_sf)
    pc, attrs = F._pairs_packed(p)
    assert torch.equal(pc, torch.cat(want, 1))
    rows = ([torch.cat(c2, 1)] if joint and with_pc2 else []) + \
        ([torch.cat(fl + ([] if joint else [torch.zeros(3, sum(n2))]), 1)] if with_sf else [])
    assert (attrs is None and not rows) or torch.equal(attrs, torch.cat(rows, 0))
    # the epilogue: an op that kept the first k_i columns of every cloud, and its attrs with them
    keep = [max(c.shape[1] - 1 - i, 0) for i, c in enumerate(want)]
    spans = [(p.prefix[i], p.prefix[i] + k) for i, k in enumerate(keep)]
    stats = torch.arange(4 * len(want)).reshape(len(want), 4)
    o1, o2, of, st = F._pairs_out(p, pc, attrs, stats, spans)
    assert all(torch.equal(o, c[:, :k]) for o, c, k in zip(o1, c1, keep)) and len(o1) == B
    assert (o2 is None) if not with_pc2 else all(torch.equal(o, c[:, :k]) for o, c, k in zip(o2, c2, keep if joint else keep[B:]))
    assert (of is None) if not with_sf else all(torch.equal(o, f[:, :k]) for o, f, k in zip(of, fl, keep))
    assert st.shape == ((len(want), 4) if joint else (2, B, 4)) and torch.equal(st.reshape(-1, 4), stats)


def test_pair_forms_take_tensors_and_refuse():
    a, b = torch.zeros(3, 10), torch.zeros(3, 12)
    p = F._pairs_in('op', torch.zeros(2, 3, 10), torch.zeros(2, 3, 10), None, True)
    assert len(p.c1) == len(p.c2) == 2 and p.prefix == [0, 10, 20] and p.joint
    p = F._pairs_in('op', a, b, a, False)
    assert p.prefix == [0, 10, 22] and not p.joint and riders(p).shape == (3, 22) and not riders(p)[:, 10:].any()
    assert len(F._pairs_in('op', [a] * 64, [a] * 64, None, True).clouds) == 64
    assert len(F._pairs_in('op', [a] * 32, [b] * 32, None, False).clouds) == 64
    many = 'op: pc1, pc2 and sf hold as many clouds, and sf as many points as pc1'
    for args, text in (((a, b, None, True), 'op: corr=True takes clouds that correspond point to point (as many points in pc1 and pc2)'),
                       ((a, a, b, True), many), ((a, None, b, True), many), (([a], [a, a], None, True), many),
                       (([a, a], None, [a], False), many),
                       (([a] * 65, None, None, False), 'op: 65 pairs (1 .. 64 a call)'),
                       (([a] * 65, [a] * 65, None, True), 'op: 65 pairs (1 .. 64 a call)'),
                       (([a] * 33, [b] * 33, None, False), 'op: 33 pairs (1 .. 32 a call)'),
                       ((torch.zeros(10, 3), None, None, True), 'op: pc1 is a (3, N) or (B, 3, N) tensor or a list of (3, N_b) tensors'),
                       ((a, [], None, True), 'op: pc2 is a (3, N) or (B, 3, N) tensor or a list of (3, N_b) tensors'),
                       ((a, a, 'x', True), 'op: sf is a (3, N) or (B, 3, N) tensor or a list of (3, N_b) tensors')):
        with pytest.raises(_lib.HplError) as e:
            F._pairs_in('op', *args)
        assert str(e.value) == text


def test_packed_pairs_reads_a_forward_in_place():
    """The forms of rigid_refine on host tensors: the (B, 3, N) view of a forward's rows and a ragged forward's row blocks are
    handed on without a copy."""
    B, n = 3, 5
    rows = torch.randn(B * n, 3)
    flow = rows.view(B, n, 3).transpose(1, 2)                                        # what a batched forward returns
    pc1 = torch.randn(B, 3, n)
    pc, fl, prefix, counts, form = F._packed_pairs(pc1, flow, None, 'op')
    assert fl.data_ptr() == rows.data_ptr() and fl.shape == (B * n, 3) and fl.is_contiguous() and form is None
    assert prefix == [0, 5, 10, 15] and counts == [5] * 3 and torch.equal(pc, torch.cat(list(pc1), 1))
    assert F._rows_as(fl, form, prefix).data_ptr() == rows.data_ptr() and torch.equal(F._rows_as(fl, form, prefix), flow)
    ns = [4, 7, 2]
    pre = F._prefix_of(ns)
    ragged = torch.randn(sum(ns), 3)
    flows = [ragged[pre[b]:pre[b + 1]].t()[None] for b in range(3)]                    # a ragged forward's (1, 3, N_b) views
    pc, fl, prefix, counts, form = F._packed_pairs(clouds_of(ns), flows, ns, 'op')
    assert fl.data_ptr() == ragged.data_ptr() and fl.shape == (sum(ns), 3) and prefix == pre and form == [True] * 3
    back = F._rows_as(fl, form, prefix)
    assert all(torch.equal(x, y) and x.data_ptr() == y.data_ptr() for x, y in zip(back, flows))
    one = torch.randn(3, 6)
    pc, fl, prefix, counts, form = F._packed_pairs(one, one, [2, 4], 'op')
    assert pc is one and fl is one and prefix == [0, 2, 6] and form is False
