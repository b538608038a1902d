"""CPU: the inference PROGRAM with the Up layers' bias-only 1x1 convs folded into their consumers' weights (DESIGN.md §23;
plan.build_program(fold=True) emits without a device, the folded weights are allocated and not computed).

Folded, an Up layer of HPLFlowNet is conv15 -> slice: no GCONV op of a trailing 1x1, no op under either HPL_COND_SHRINK
condition, every Up input below the deepest level four columns wider with a C == 8 el_minus_gr copy, conv2 on 1024 pre-1x1
channels with a folded bias.  Unfolded (build_program's default, what TrainPlan and HPL_FOLD_UP=0 take) the op list is the one
of before the fold: 122 / 64 forward ops (tests/test_train_plan_cpu.py pins the same numbers) with both Up orders.  The shallow
model has single-conv Up stacks: nothing to fold."""
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OP_GCONV, OP_SLICE, OP_COPY = 1, 3, 4
TBL_NONE, TBL_BLUR0 = 0, 2


def _model(arch, bias=True):
    import hplflownet_amd as H
    from hplflownet_amd.synthetic import SCALES_FILTER_MAP
    nl = 7 if arch == 'HPLFlowNet' else 5
    a = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP[:nl], evaluate=False, use_leaky=True, bcn_use_bias=bias,
                              bcn_use_norm=True, last_relu=False, DEVICE='cpu')
    return getattr(H, arch)(a)


def _program(model, fold):
    from hplflownet_amd import ops
    from hplflownet_amd.plan import build_program
    return build_program(model, ops.WeightBank(), fold=fold)


def _sig(P):
    """What an op does, without pointers: comparable between two emissions."""
    return [(o.kind, o.a.buf, o.a.col_off, o.a.cols, o.out.buf, o.out.col_off, o.out.cols, o.m_sym, o.level, o.table, o.order,
             o.F, o.C, o.N, o.weight, o.bias, o.act, o.cond, o.cond_level, o.flags) for o in P.ops]


def test_folded_program_of_hplflownet():
    m = _model('HPLFlowNet')
    assert m.fold_up()
    U, Fd = _program(m, False), _program(m, True)
    # the folded Up convs are read by a slice: none asks for the largest magnitude of its result (HPL_FLAG_NOYAMAX = 64)
    assert all(o.flags & 64 for o in Fd.ops if o.kind == OP_GCONV and o.table == TBL_BLUR0)
    assert not any(o.flags & 64 for o in U.ops)
    assert len(U.ops) == 122 and not U.folds and len(Fd.folds) == 7
    # no op under either SHRINK condition; the unfolded form has both orders of all seven Up layers
    assert all(o.cond == 0 for o in Fd.ops)
    assert sum(1 for o in U.ops if o.cond == 1) == 7 * 3 and sum(1 for o in U.ops if o.cond == 2) == 7 * 3
    # the Up convs: one 15-tap GCONV per level, no dense GCONV fed by one (the trailing 1x1 is gone)
    up = [o for o in Fd.ops if o.kind == OP_GCONV and o.table == TBL_BLUR0]
    assert len(up) == 7 and all(o.F == 15 for o in up)
    up_out = set(o.out.buf for o in up)
    assert not [o for o in Fd.ops if o.kind == OP_GCONV and o.table == TBL_NONE and o.a.buf in up_out]
    slices = [o for o in Fd.ops if o.kind == OP_SLICE]
    assert len(slices) == 7 and all(o.bias == -1 and o.a.buf in up_out for o in slices)
    # every Up input below the deepest level: 4 columns wider, el_minus_gr | 1, 0, 0, 0 by one C == 8 copy
    widths = {o.level: o.C for o in up}
    for L in range(7):
        layer = getattr(m, 'bcn%d_' % (L + 1))
        assert widths[L] == layer.num_input + (4 if L < 6 else 0), (L, widths[L])
    c8 = [o for o in Fd.ops if o.kind == OP_COPY and o.a.buf == -1 and o.C == 8]
    assert len(c8) == 6 and sorted(o.level for o in c8) == [1, 2, 3, 4, 5, 6]
    assert all(o.out.col_off == 0 and o.out.cols == 8 and o.out.buf in set(u.a.buf for u in up) for o in c8)
    assert not [o for o in U.ops if o.kind == OP_COPY and o.C == 8]
    # the head: conv2 on bcn1_'s 1024 pre-1x1 channels, its bias the folded one
    conv2 = [o for o in Fd.ops if o.kind == OP_GCONV and o.table == TBL_NONE and o.a.buf == slices[-1].out.buf]
    assert len(conv2) == 1 and (conv2[0].C, conv2[0].N, conv2[0].act) == (1024, 1024, 1)
    assert Fd.biases[conv2[0].bias] is Fd.folds[0].bias
    # 7 x (1 conv + 1 slice) instead of 7 x (2 x 3 ops); everything else op for op
    assert len(Fd.ops) == 122 - 7 * 4
    shapes = [tuple(f.weight.shape) for f in Fd.folds]
    assert shapes[0] == (1024, 1024, 1) and shapes[1] == (1024, 584, 15, 1) and shapes[2] == (512, 328, 15, 1)


def test_no_bias_no_ones_part():
    m = _model('HPLFlowNet', bias=False)
    for L in range(7):                    # a bias-free trailing conv as well: nothing left to carry
        getattr(m, 'bcn%d_' % (L + 1)).blur_conv[-1].bias = None
    Fd = _program(m, True)
    up = {o.level: o.C for o in Fd.ops if o.kind == OP_GCONV and o.table == TBL_BLUR0}
    assert all(up[L] == getattr(m, 'bcn%d_' % (L + 1)).num_input for L in range(7))
    assert not [o for o in Fd.ops if o.kind == OP_COPY and o.C == 8]
    assert all(f.args[3] == -1 for f in Fd.folds)
    # the conv's own bias alone still takes the ones part
    m2 = _model('HPLFlowNet', bias=False)
    assert len([o for o in _program(m2, True).ops if o.kind == OP_COPY and o.C == 8]) == 6


def test_train_program_is_unfolded():
    """TrainPlan._program, run on a stub that carries what it reads of a TrainPlan (no device): the forward part of the training
    program is the unfolded op list, op for op, although model.fold_up() is True."""
    import collections
    import torch
    from hplflownet_amd import ops
    from hplflownet_amd.train_plan import TrainPlan
    m = _model('HPLFlowNet')
    assert m.fold_up()
    stub = types.SimpleNamespace(bank=ops.WeightBank(), params=[p for p in m.parameters()], gflat=torch.zeros(1),
                                 _goff=collections.defaultdict(int), reducer=types.SimpleNamespace(buckets=[None]),
                                 _bucket_of=collections.defaultdict(int))
    P = TrainPlan._program(stub, m)
    P = P if P is not None else stub._B.P
    assert stub.n_fwd == 122 and not P.folds
    assert _sig(P)[:stub.n_fwd] == _sig(_program(m, False))


def test_a_trailing_1x1_that_is_not_square_is_not_folded():
    """The fold keeps the width of the `up` block: a model whose trailing 1x1 changes the width runs unfolded."""
    import hplflownet_amd as H
    from hplflownet_amd.synthetic import SCALES_FILTER_MAP
    odd_cls = type('OddUp', (H.HPLFlowNet,), {'UP': dict(list(H.HPLFlowNet.UP.items()) + [(6, [96, 128])])})
    a = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP[:7], evaluate=False, use_leaky=True, bcn_use_bias=True,
                              bcn_use_norm=True, last_relu=False, DEVICE='cpu')
    odd = odd_cls(a)
    assert not odd.fold_up() and len(_program(odd, odd.fold_up()).ops) == 122


def test_shallow_model_is_unchanged():
    m = _model('HPLFlowNetShallow')
    assert not m.fold_up()
    U = _program(m, False)
    assert len(U.ops) == 64 and _sig(U) == _sig(_program(m, m.fold_up()))


def test_switch_off_gives_the_unfolded_program():
    """HPL_FOLD_UP=0 is read once by the package: a child process sees fold_up() False for HPLFlowNet, and the program a plan
    would build (build_program(fold=model.fold_up())) is the unfolded one, op for op."""
    import json
    code = ('import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
            'import test_fold_up_cpu as T\n'
            'from hplflownet_amd import ops\n'
            'm = T._model("HPLFlowNet")\n'
            'P = T._program(m, m.fold_up())\n'
            'print(json.dumps([ops.FOLD_UP, m.fold_up(), len(P.folds), T._sig(P)]))\n') % (ROOT, os.path.join(ROOT, 'tests'))
    env = dict(os.environ, HPL_FOLD_UP='0')
    out = json.loads(subprocess.check_output([sys.executable, '-c', code], env=env).decode().splitlines()[-1])
    assert out[:3] == [False, False, 0]
    want = json.loads(json.dumps(_sig(_program(_model('HPLFlowNet'), False))))
    assert len(want) == 122 and out[3] == want
