"""CPU: the host side of the self-supervised loss in the native training step -- the refusals of hpl_pair_grad
and hpl_plan_run_range_loss without a device, the loss argument of TrainPlan.step_batch, and the --selfsup-native flag."""
import ctypes
import types

import pytest
import torch

from hplflownet_amd import _lib, engine
from hplflownet_amd.train_plan import TrainPlan

BIG = ((1 << 31) + 2) // 3                      # the first refused row count (rows >= 2^31 / 3)


def z(*s, **k):
    return torch.zeros(*s, **k)


def _prefix(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_pair_grad_refuses_without_a_device():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()                 # (host memory: every call below is refused before it would launch)
    p = ctypes.addressof(buf)

    def grad(dflow=p, rows=100, batch=2, pair_loss=p, stride=4, g=p, loss=p):
        rc = lib.hpl_pair_grad(dflow, rows, batch, pair_loss, stride, g, loss, None)
        assert rc != -1 or lib.hpl_last_error().startswith(b'hpl_pair_grad'), lib.hpl_last_error()
        return rc

    for kw in (dict(batch=0), dict(batch=65), dict(batch=-3), dict(g=None, loss=None), dict(dflow=None), dict(pair_loss=None),
               dict(stride=0), dict(rows=-1), dict(rows=BIG), dict(rows=1 << 60),
               dict(dflow=p + 2), dict(g=p + 1), dict(pair_loss=p + 3), dict(loss=p + 2)):
        assert grad(**kw) == -1, kw
    assert grad(rows=0, loss=None) == 0              # nothing to launch
    assert grad(rows=0, loss=None, pair_loss=None) == 0


def test_plan_run_range_loss_refuses_without_a_device():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    lv = (_lib.LevelTables * 1)()
    lv[0].n0, lv[0].n1, lv[0].H0, lv[0].H1 = 100, 100, 50, 50
    op, bufs = (_lib.Op * 1)(), (_lib.Buf * 1)()
    bufs[0].rows_sym, bufs[0].cols = 0, 4
    plan = lib.hpl_plan_create(op, 1, bufs, 1, None, 0, None, 0)          # (host bookkeeping only)
    assert plan

    def run(kind, batch, prefix, stride=4, plan=plan):
        return lib.hpl_plan_run_range_loss(plan, lv, 1, p, p, p, p, p, p, 1 << 20, None, None, 0, 0, 1, kind, batch, prefix, p,
                                           stride, p)
    assert run(2, 2, _prefix(0, 40, 100), plan=None) == -1               # (a null plan: as hpl_plan_run_range)
    for kind, batch, prefix, stride in ((1, 2, _prefix(0, 40, 100), 4), (3, 2, _prefix(0, 40, 100), 4),      # no such loss
                                        (-1, 2, _prefix(0, 40, 100), 4),
                                        (2, 0, _prefix(0, 100), 4), (2, 65, _prefix(*range(66)), 4),           # batch outside 1 .. 64
                                        (2, 2, None, 4),                                                       # no prefix
                                        (2, 2, _prefix(0, 40, 100), 0),                                        # no stride
                                        (2, 2, _prefix(0, 40, 99), 4), (2, 2, _prefix(0, 40, 101), 4),         # not the lattice's points
                                        (2, 2, _prefix(1, 40, 100), 4)):
        assert run(kind, batch, prefix, stride) == -1, (kind, batch)
        assert lib.hpl_last_error().startswith(b'hpl_plan_run_range_loss'), lib.hpl_last_error()
    lib.hpl_plan_destroy(plan)


def test_step_batch_loss_argument_launches_nothing():
    plan = TrainPlan.__new__(TrainPlan)                                   # no model, no device: a launch would fail differently
    lat2 = types.SimpleNamespace(batch=2)
    good = (z(2, 3, 9), z(2, 3, 7))
    with pytest.raises(_lib.HplError):
        plan.step_batch(*good, z(2, 3, 9), lat2, loss='l2')              # no such loss
    for args in ((z(3, 9), z(3, 7), None, lat2),                          # not a batch
                 (z(2, 3, 9), z(3, 3, 7), None, lat2),                    # pair counts differ
                 (*good, z(2, 3, 7), lat2),                               # a label of another shape (never read, still checked)
                 (*good, None, types.SimpleNamespace(batch=3)),           # lattice of another batch
                 (*good, None, types.SimpleNamespace(batch=2, ragged=True, point_counts=[(9, 7)] * 2))):     # a ragged lattice
        with pytest.raises(_lib.HplError):
            plan.step_batch(*args, loss='selfsup')


def test_selfsup_native_flag():
    for argv in (['--selfsup-native'], ['--selfsup-native', '--loss', 'epe3d'], ['--selfsup-native', '--loss', 'selfsup', '--evaluate']):
        with pytest.raises(SystemExit):
            engine.main(argv)
    a = engine.parse_args(['--loss', 'selfsup', '--selfsup-native', '--train-batch-size', '2'])
    assert a.selfsup_native and a.train_batch_size == 2
    assert not engine.parse_args([]).selfsup_native and not engine.parse_args(['--loss', 'selfsup']).selfsup_native
