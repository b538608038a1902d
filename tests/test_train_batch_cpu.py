"""CPU: the host side of batched training -- the --train-batch-size argument, how training batches are grouped, the argument
checks of the batched step (HplError before anything is launched) and the null-argument returns of its two C entry points."""
import ctypes
import types

import pytest
import torch

from hplflownet_amd import _lib, data as data_mod, engine
from hplflownet_amd.lattice import LatticePipeline
from hplflownet_amd.train_plan import TrainPlan, check_batch_step


def test_train_batch_size_argument():
    for argv in (['--train-batch-size', '0'], ['--train-batch-size', '65'], ['--evaluate', '--train-batch-size', '2'],
                 ['--evaluate', '--train-batch-size', '1']):
        with pytest.raises(SystemExit):
            engine.main(argv)


class Reader(object):
    def __init__(self, counts, with_counts):
        self.counts, self.fetched = counts, []
        if with_counts:
            self.point_counts = lambda i: self.counts[i]

    def __len__(self):
        return len(self.counts)

    def __getitem__(self, i):
        self.fetched.append(i)
        n1, n2 = self.counts[i]
        return torch.zeros(3, n1), torch.zeros(3, n2), torch.zeros(3, n1)


def test_training_batches_group_equal_counts():
    c = [(512, 512)] * 3 + [(400, 512)] + [(512, 512)] * 4
    order = [7, 6, 5, 4, 3, 2, 1, 0]
    with_counts = Reader(c, True)
    counts = [engine.point_counts(with_counts, k) for k in order]
    assert with_counts.fetched == []                              # a reader that knows its counts is not fetched for them
    assert engine.batch_groups(counts, 2) == [[0, 1], [2, 3], [4], [5, 6], [7]]
    plain = Reader(c, False)
    assert [engine.point_counts(plain, k) for k in order] == counts
    shard = engine._Shard(with_counts, 1, 2)                     # samples 1, 3, 5, 7
    assert [shard.point_counts(i) for i in range(len(shard))] == [c[1], c[3], c[5], c[7]]
    syn = engine.SyntheticPairs.__new__(engine.SyntheticPairs)
    syn.items = [(torch.zeros(3, 9), torch.zeros(3, 7), torch.zeros(3, 9))]
    assert tuple(syn.point_counts(0)) == (9, 7)
    # the training protocol's transform fixes the counts: a folder answers without loading a sample
    folder = data_mod._PairFolder(data_mod.Augmentation(engine.AUG_TOGETHER, engine.AUG_PC2, engine.DATA_PROCESS, 2048, False))
    folder.samples = ['never-loaded']
    assert folder.point_counts(0) == (2048, 2048)


def test_pipeline_batches_for_training():
    gen = types.SimpleNamespace()
    with pytest.raises(_lib.HplError):
        LatticePipeline(gen, None, 0, 4, for_training=True, native=False, batch=2)       # the staged driver builds one pair
    with pytest.raises(_lib.HplError):
        LatticePipeline(gen, None, 0, 4, for_training=True, native=True, batch=2, groups=[[0, 1, 2], [3]])
    p = LatticePipeline(gen, None, 0, 5, for_training=True, native=True, batch=2, groups=[[0, 1], [2], [3, 4]])
    assert p._end - p._first == 3
    p = LatticePipeline(gen, None, 0, 5, for_training=True, native=True, batch=2)
    assert p._groups == [[0, 1], [2, 3], [4]]


def z(*s):
    return torch.zeros(*s)


def test_batched_step_checks_launch_nothing():
    lat2 = types.SimpleNamespace(batch=2)
    good = (z(2, 3, 9), z(2, 3, 7), z(2, 3, 9))
    assert check_batch_step(*good, lat2) == 2
    assert check_batch_step(z(1, 3, 9), z(1, 3, 7), z(1, 3, 9), types.SimpleNamespace()) == 1
    bad = [(z(3, 9), z(3, 7), z(3, 9), lat2),                          # not a batch
           (z(2, 3, 9), z(3, 3, 7), z(2, 3, 9), lat2),                 # pair counts differ
           (z(2, 3, 9), z(2, 3, 7), z(2, 3, 7), lat2),                 # sf not pc1's shape
           (z(2, 4, 9), z(2, 4, 7), z(2, 4, 9), lat2),                 # not 3-d points
           (*good, types.SimpleNamespace(batch=3)),                    # lattice of another batch
           (*good, types.SimpleNamespace())]                           # a single-pair lattice
    tr = engine.Trainer.__new__(engine.Trainer)                        # no model, no device: a launch would fail differently
    plan = TrainPlan.__new__(TrainPlan)
    for args in bad:
        for f in (check_batch_step, tr.train_step_batch, plan.step_batch):
            with pytest.raises(_lib.HplError):
                f(*args)


def test_batched_training_entry_points_validate_without_gpu():
    lib = _lib.load()
    assert lib.hpl_batch_stage(2, 10, 10, None, None, None, None, None, None, None) == -1
    assert b'hpl_batch_stage' in lib.hpl_last_error()
    buf = (ctypes.c_float * 16)()                 # (host memory: every call below is refused before it would launch)
    p = ctypes.addressof(buf)
    assert lib.hpl_batch_stage(0, 10, 10, p, p, None, p, p, None, None) == -1            # no pairs
    assert lib.hpl_batch_stage(2, 10, 10, p, p, p, p, p, None, None) == -1                # sf without a destination
    assert lib.hpl_epe3d_pairs(None, None, 2, 10, None, None) == -1
    assert b'hpl_epe3d_pairs' in lib.hpl_last_error()
    assert lib.hpl_epe3d_pairs(p, p, 65, 10, p, None) == -1
    assert lib.hpl_epe3d_pairs(p, p, 2, 0, p, None) == -1
