"""CPU: the argument checks of batched inference that run before any launch (batch sizes, pc1 / pc2 / lattice agreement,
training refusing a batch), the engine's grouping of pairs by point count, and the batched entry points of the C ABI."""
import types

import pytest
import torch

from hplflownet_amd import _lib, engine
from hplflownet_amd.flownet import batch_of
from hplflownet_amd.lattice import MAX_BATCH, check_batch, to_reference_format


def test_batch_argument_checks():
    z = lambda *s: torch.zeros(*s)            # noqa: E731
    assert check_batch(z(3, 3, 100), z(3, 3, 70)) == 3          # N1 != N2 is allowed
    assert check_batch(z(1, 3, 8), z(1, 3, 8)) == 1
    assert check_batch(z(MAX_BATCH, 3, 8), z(MAX_BATCH, 3, 8)) == MAX_BATCH
    for a, b in [(z(3, 3, 10), z(2, 3, 10)),                      # mismatched B
                 (z(0, 3, 10), z(0, 3, 10)),                      # B = 0
                 (z(MAX_BATCH + 1, 3, 4), z(MAX_BATCH + 1, 3, 4)),
                 (z(3, 10), z(3, 10)),                            # not a batch
                 (z(2, 4, 10), z(2, 4, 10)),                      # not xyz
                 (z(2, 3, 0), z(2, 3, 0))]:
        with pytest.raises(_lib.HplError):
            check_batch(a, b)


def test_forward_batch_agreement():
    single, batched = types.SimpleNamespace(), types.SimpleNamespace(batch=4)
    z = torch.zeros
    assert batch_of(z(1, 3, 9), z(1, 3, 9), single, grad=True) == 1
    assert batch_of(z(3, 9), z(3, 9), single, grad=False) == 1
    assert batch_of(z(4, 3, 9), z(4, 3, 7), batched, grad=False) == 4
    for args in [(z(4, 3, 9), z(4, 3, 9), single, False),          # (B, 3, N) inputs, single-pair lattice
                 (z(1, 3, 9), z(1, 3, 9), batched, False),          # batched lattice, one pair of inputs
                 (z(4, 3, 9), z(2, 3, 9), batched, False),          # pc1 / pc2 disagree
                 (z(4, 3, 9), z(4, 3, 9), batched, True)]:          # autograd (training) on a batch
        with pytest.raises(_lib.HplError):
            batch_of(*args)
    with pytest.raises(_lib.HplError):
        batch_of(z(4, 3, 9), z(4, 3, 9), batched, False, pair_batched=False)


def test_reference_format_and_training_refuse_a_batch():
    lat = types.SimpleNamespace(batch=3, levels=[])
    with pytest.raises(_lib.HplError):
        to_reference_format(lat)
    tr = engine.Trainer.__new__(engine.Trainer)          # host-side check: nothing is launched
    with pytest.raises(_lib.HplError):
        tr.train_step(None, None, None, lat)


def test_engine_groups_pairs_by_point_count():
    g = engine.batch_groups
    c = [(8192, 8192)] * 5
    assert g(c, 1) == [[0], [1], [2], [3], [4]]
    assert g(c, 2) == [[0, 1], [2, 3], [4]]
    assert g(c, 8) == [[0, 1, 2, 3, 4]]
    # a short frame (allow_less_points) runs in a batch of its own, its neighbours around it
    c = [(8192, 8192), (8192, 8192), (6000, 8192), (8192, 8192), (8192, 8192), (8192, 8192), (8192, 7000)]
    assert g(c, 4) == [[0, 1], [2], [3, 4, 5], [6]]
    assert g([], 4) == []

    class Reader(object):               # _batches fetches each sample once, in order, with the same grouping
        def __init__(self, counts):
            self.counts, self.fetched = counts, []

        def __len__(self):
            return len(self.counts)

        def __getitem__(self, i):
            self.fetched.append(i)
            n1, n2 = self.counts[i]
            return torch.zeros(3, n1), torch.zeros(3, n2), torch.zeros(3, n1)
    r = Reader(c)
    groups = list(engine.Trainer._batches(r, 4))
    assert r.fetched == list(range(len(c)))
    assert [len(x) for x in groups] == [len(x) for x in g(c, 4)]


def test_engine_batch_size_argument():
    with pytest.raises(SystemExit):
        engine.main(['--batch-size', '4'])                    # training takes one pair per step
    with pytest.raises(SystemExit):
        engine.main(['--evaluate', '--batch-size', '65'])


def test_batched_entry_points_validate_without_gpu():
    lib = _lib.load()
    assert lib.hpl_lattice_begin_batch(None, None, None, 2, 10, 10, None, 0, None) == -1
    assert b'bad arguments' in lib.hpl_last_error()
    assert lib.hpl_lattice_arena_bytes_batch(None, 2, 10, 10) == -1
    assert lib.hpl_lattice_pair_counts(None, None) == -1
    assert lib.hpl_plan_run_batch(None, None, 1, 2, None, None, None, None, 0, None) == -1
    assert lib.hpl_plan_batch_extra_bytes(None, 0) == -1
