"""CPU: the argument checks of ragged batched inference that run before any launch (list lengths, batch sizes, cloud shapes,
devices and dtypes, pc1 / pc2 / lattice agreement, training refusing a ragged lattice), the engine's ragged grouping, and
the ragged entry points of the C ABI."""
import types

import pytest
import torch

from hplflownet_amd import _lib, engine
from hplflownet_amd.flownet import batch_of
from hplflownet_amd.lattice import MAX_BATCH, MAX_RAGGED_POINTS, check_ragged, to_reference_format


def z(*s, **k):
    return torch.zeros(*s, **k)


def test_ragged_argument_checks():
    assert check_ragged([z(3, 100), z(3, 7)], [z(3, 70), z(3, 9)]) == (2, [(100, 70), (7, 9)])
    assert check_ragged((z(3, 5),), (z(3, 5),)) == (1, [(5, 5)])
    assert check_ragged([z(3, 1)] * MAX_BATCH, [z(3, 2)] * MAX_BATCH)[0] == MAX_BATCH
    for a, b in [([z(3, 10), z(3, 10)], [z(3, 10)]),              # list lengths differ
                 ([], []),                                          # B = 0
                 ([z(3, 4)] * (MAX_BATCH + 1), [z(3, 4)] * (MAX_BATCH + 1)),
                 ([z(3, 10), z(2, 3, 10)], [z(3, 10), z(3, 10)]),   # a cloud that is not (3, N)
                 ([z(4, 10)], [z(4, 10)]),                          # not xyz
                 ([z(3, 10), z(3, 0)], [z(3, 10), z(3, 5)]),        # N = 0
                 ([z(3, 10), z(3, 10, dtype=torch.float64)], [z(3, 10), z(3, 10)]),       # mixed dtypes
                 ([z(3, 10), z(3, 10, dtype=torch.float16)], [z(3, 10), z(3, 10, dtype=torch.float16)]),
                 ([z(3, 10), z(3, 10, device='meta')], [z(3, 10), z(3, 10)]),             # mixed devices
                 (z(2, 3, 10), [z(3, 10), z(3, 10)]),               # a tensor and a list
                 ([z(3, MAX_RAGGED_POINTS), z(3, 1)], [z(3, 1), z(3, 1)])]:              # a side above the 32-bit budget
        with pytest.raises(_lib.HplError):
            check_ragged(a, b)


def test_forward_ragged_agreement():
    single = types.SimpleNamespace()
    ragged = types.SimpleNamespace(batch=2, ragged=True, point_counts=[(9, 7), (5, 5)])
    equal = types.SimpleNamespace(batch=2)
    assert batch_of([z(3, 9), z(3, 5)], [z(3, 7), z(3, 5)], ragged, grad=False) == 2
    assert batch_of([z(3, 9)], [z(3, 9)], single, grad=True) == 1                 # one pair in lists: the single-pair lattice
    assert batch_of(z(1, 3, 9), z(1, 3, 9), single, grad=True) == 1               # the tensor forms keep their rules
    assert batch_of(z(2, 3, 9), z(2, 3, 9), equal, grad=False) == 2
    for args in [([z(3, 9), z(3, 5)], [z(3, 7)], ragged, False),                  # list lengths differ
                 ([z(3, 9), z(3, 5)], [z(3, 7), z(3, 5)], single, False),         # lists, single-pair lattice
                 ([z(3, 9), z(3, 5)], [z(3, 7), z(3, 5)], equal, False),          # lists, equal-count batch
                 ([z(3, 5), z(3, 9)], [z(3, 5), z(3, 7)], ragged, False),         # counts of other pairs
                 ([z(3, 9), z(3, 5)], z(2, 3, 5), ragged, False),                 # a list and a tensor
                 (z(2, 3, 9), z(2, 3, 9), ragged, False),                         # tensors with a ragged lattice
                 ([z(3, 9), z(3, 5)], [z(3, 7), z(3, 5)], ragged, True)]:         # autograd on a ragged batch
        with pytest.raises(_lib.HplError):
            batch_of(*args)
    with pytest.raises(_lib.HplError):
        batch_of([z(3, 9), z(3, 5)], [z(3, 7), z(3, 5)], ragged, False, pair_batched=False)


def test_training_and_wire_format_refuse_a_ragged_lattice():
    from hplflownet_amd.train_plan import TrainPlan, check_batch_step
    lat = types.SimpleNamespace(batch=2, ragged=True, point_counts=[(8, 8), (8, 8)], levels=[])
    p = z(2, 3, 8)
    with pytest.raises(_lib.HplError):
        to_reference_format(lat)
    with pytest.raises(_lib.HplError):
        check_batch_step(p, p, p, lat)                      # equal counts, but the lattice is ragged
    tr = engine.Trainer.__new__(engine.Trainer)            # host-side checks: nothing is launched
    with pytest.raises(_lib.HplError):
        tr.train_step(None, None, None, lat)
    with pytest.raises(_lib.HplError):
        tr.train_step_batch(p, p, p, lat)
    tp = TrainPlan.__new__(TrainPlan)
    with pytest.raises(_lib.HplError):
        tp.step_batch(p, p, p, lat)
    with pytest.raises(_lib.HplError):
        tp.step(p[0], p[0], p[0], lat)


def test_engine_ragged_groups():
    g = engine.ragged_groups
    c = [(8192, 8192), (5000, 8192), (8192, 8192), (4100, 4100), (8192, 7000)]
    assert g(c, 1) == [[0], [1], [2], [3], [4]]
    assert g(c, 2) == [[0, 1], [2, 3], [4]]
    assert g(c, 8) == [[0, 1, 2, 3, 4]]                     # counts do not split a group
    # the points-per-side budget closes a group before it would overflow, on either side
    assert g(c, 8, budget=16384) == [[0, 1], [2, 3], [4]]              # (a group may fill the budget exactly)
    assert g(c, 8, budget=16383) == [[0], [1], [2, 3], [4]]
    assert g([(10, 90), (10, 20), (10, 1)], 8, budget=100) == [[0], [1, 2]]
    assert g([(200, 1), (5, 5)], 4, budget=100) == [[0], [1]]           # a pair above the budget runs alone
    big = [(8192, 8192)] * 40
    groups = g(big, 64)
    assert [len(x) for x in groups] == [16, 16, 8]                      # the default budget: B x N <= 131 072
    assert engine.RAGGED_POINT_BUDGET == 131072
    assert g([], 4) == []
    # every sample in exactly one group, in order
    c = [(1000 + 37 * i % 700, 900 + 11 * i % 300) for i in range(50)]
    for B in (1, 3, 8, 64):
        for budget in (2000, 5000, 131072):
            groups = g(c, B, budget)
            assert sum(groups, []) == list(range(50))
            for x in groups:
                assert 1 <= len(x) <= B
                if len(x) > 1:
                    assert sum(c[i][0] for i in x) <= budget and sum(c[i][1] for i in x) <= budget


def test_engine_ragged_batches_fetch_each_sample_once_in_order():
    class Reader(object):
        def __init__(self, n):
            self.n, self.fetched = n, []

        def __len__(self):
            return len(self.n)

        def __getitem__(self, i):
            self.fetched.append(i)
            return z(3, self.n[i][0]), z(3, self.n[i][1]), z(3, self.n[i][0])
    counts = [(300, 200), (100, 100), (250, 400), (50, 60), (500, 500), (10, 10), (20, 20)]
    for B, budget in ((2, 10 ** 6), (4, 600), (8, 700)):
        r = Reader(counts)
        groups = list(engine.Trainer._ragged_batches(r, B, budget))
        assert r.fetched == list(range(len(counts)))
        sizes = [[(int(s[0].shape[-1]), int(s[1].shape[-1])) for s in grp] for grp in groups]
        want = engine.ragged_groups(counts, B, budget)
        assert sizes == [[counts[i] for i in grp] for grp in want]


def test_engine_ragged_flag():
    with pytest.raises(SystemExit):
        engine.main(['--ragged'])                            # training: no
    with pytest.raises(SystemExit):
        engine.main(['--evaluate', '--ragged'])              # --batch-size 1: nothing to batch


def test_ragged_abi_refuses_bad_arguments():
    import ctypes
    L = _lib.load()
    n = (ctypes.c_int64 * 2)(8, 8)
    assert L.hpl_lattice_arena_bytes_ragged(None, 2, n, n) == -1
    assert L.hpl_lattice_begin_ragged(None, None, None, 2, n, n, None, 0, None) == -1
    p = (ctypes.c_void_p * 2)(16, 32)
    ld = (ctypes.c_int64 * 2)(8, 8)
    bad = (ctypes.c_int64 * 2)(8, 0)
    assert L.hpl_ragged_stage(0, p, n, ld, p, n, ld, None, None, 64, 64, None, None) == -1       # B = 0
    assert L.hpl_ragged_stage(65, p, n, ld, p, n, ld, None, None, 64, 64, None, None) == -1      # B = 65
    assert L.hpl_ragged_stage(2, p, bad, ld, p, n, ld, None, None, 64, 64, None, None) == -1     # N = 0
    short = (ctypes.c_int64 * 2)(8, 4)
    assert L.hpl_ragged_stage(2, p, n, short, p, n, ld, None, None, 64, 64, None, None) == -1    # row stride < N
