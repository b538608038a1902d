"""CPU: hpl_knn_interp's declaration, export and refusals (no device needed), and the numpy restatement tests/knn_oracle.py
against a float64 brute force, with the exact-hit and tie rules on constructed duplicates."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT
from hplflownet_amd import _lib
from knn_oracle import brute_force64, interpolate64, knn_search

I64 = ctypes.c_int64


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_knn_interp\s*\(', body)
    assert 'hpl_knn_interp' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'hpl_knn_interp')
    from hplflownet_amd import build
    assert 'knn_interp.hip' in build.SOURCES


def call(ref=8, ref_ld=100, val=8, C=3, q=8, q_ld=50, k=3, eps=1e-8, batch=1, rp=(0, 100), qp=(0, 50), idx=None, dist2=None,
         out=8, cov=None):
    """hpl_knn_interp with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    lib = _lib.load()
    rp = (I64 * len(rp))(*rp) if rp is not None else None
    qp = (I64 * len(qp))(*qp) if qp is not None else None
    return lib.hpl_knn_interp(ref, ref_ld, val, C, q, q_ld, k, eps, batch, rp, qp, idx, dist2, out, cov, None)


@pytest.mark.parametrize('kw', [
    dict(k=0), dict(k=9), dict(k=-1), dict(C=0), dict(C=17), dict(batch=0), dict(batch=65, rp=(0,) * 66, qp=(0,) * 66),
    dict(eps=-1e-8), dict(eps=float('inf')), dict(eps=float('nan')),
    dict(batch=2, rp=(0, 60, 50), qp=(0, 20, 50)), dict(batch=2, rp=(0, 60, 100), qp=(0, 60, 50)),
    dict(rp=(1, 100)), dict(qp=(1, 50)),
    dict(ref=None), dict(val=None), dict(q=None), dict(out=None), dict(rp=None), dict(qp=None),
    dict(qp=(0, 2 ** 31 // 3 + 1), q_ld=2 ** 31), dict(rp=(0, 2 ** 31 // 3 + 1), ref_ld=2 ** 31),
    dict(qp=(0, 2 ** 28), q_ld=2 ** 28, C=1, k=8), dict(qp=(0, 2 ** 27), q_ld=2 ** 27, C=16, k=1),
    dict(qp=(0, 2 ** 60), q_ld=2 ** 60), dict(rp=(0, 2 ** 62), ref_ld=2 ** 62), dict(ref_ld=99), dict(q_ld=49), dict(batch=2, rp=(0, 0, 100), qp=(0, 10, 50)), dict(ref=6),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_refusals_without_a_device(kw):
    assert call(**kw) == -1                                   # HPL_EINVAL
    assert b'hpl_knn_interp' in _lib.load().hpl_last_error()


def test_empty_query_set_is_a_no_op():
    """Q = 0 returns HPL_OK before any launch."""
    assert call(qp=(0, 0), q_ld=0) == 0


def test_wrapper_refuses_before_the_library():
    from hplflownet_amd import ops
    ref, val, q = torch.zeros(3, 10), torch.zeros(10, 3), torch.zeros(3, 5)
    with pytest.raises(_lib.HplError):
        ops.knn_interpolate(ref, val, q)                      # host tensors: no CPU fallback
    with pytest.raises(_lib.HplError):
        ops.knn_interpolate(ref, val, q, k=0)


@pytest.mark.parametrize('k', [1, 3, 8])
def test_restatement_against_float64(k):
    rng = np.random.RandomState(k)
    ref = rng.uniform(-10, 10, (3, 2048)).astype(np.float32)
    q = rng.uniform(-12, 12, (3, 5000)).astype(np.float32)
    idx, d2 = knn_search(ref, q, k)
    want = brute_force64(ref, q, k)
    rel = np.abs(d2.astype(np.float64) - want) / want
    print('k = %d: max relative error of the float32 d2 %.3g (bar %.3g)' % (k, rel.max(), 4 * 2.0 ** -24))
    assert rel.max() <= 4 * 2.0 ** -24
    assert (np.diff(d2, axis=0) >= 0).all() and (idx >= 0).all()
    # the listed neighbours are those distances
    own = ((q.astype(np.float64)[:, None, :] - ref.astype(np.float64)[:, idx]) ** 2).sum(0)
    assert (np.abs(own - d2) <= 4 * 2.0 ** -24 * own).all()


def test_ties_exact_hits_and_short_pairs():
    rng = np.random.RandomState(0)
    ref = rng.uniform(-1, 1, (3, 64)).astype(np.float32)
    ref[:, 40] = ref[:, 7]                                    # duplicates: 7 and 40, 3 and 5 and 60
    ref[:, 5] = ref[:, 3]
    ref[:, 60] = ref[:, 3]
    val = rng.uniform(-1, 1, (64, 3)).astype(np.float32)
    q = np.stack([ref[:, 7], ref[:, 3], ref[:, 40], ref[:, 20]], 1)
    idx, d2 = knn_search(ref, q, 3)
    assert idx[:2, 0].tolist() == [7, 40] and idx[:, 1].tolist() == [3, 5, 60] and idx[:2, 2].tolist() == [7, 40]
    assert (d2[:2, 0] == 0).all() and (d2[:, 1] == 0).all() and idx[0, 3] == 20
    out = interpolate64(val, idx, d2, 1e-8)
    assert np.array_equal(out[0], val[7].astype(np.float64)) and np.array_equal(out[1], val[3].astype(np.float64))
    assert np.array_equal(out[2], val[7].astype(np.float64)) and np.array_equal(out[3], val[20].astype(np.float64))
    # a mirrored pair of points at the same distance: the smaller index first
    ref2 = np.array([[1, -1, 0.5], [0, 0, 0], [0, 0, 0]], np.float32)
    idx, d2 = knn_search(ref2, np.zeros((3, 1), np.float32), 3)
    assert idx[:, 0].tolist() == [2, 0, 1] and d2[1, 0] == d2[2, 0]
    # two pairs, the second with 2 points only: missing entries are -1 / +inf and take no part
    idx, d2 = knn_search(ref[:, :10], q, 3, [0, 8, 10], [0, 2, 4])
    assert (idx[:, :2] < 8).all() and (idx[:, :2] >= 0).all()
    assert sorted(idx[:2, 2].tolist()) == [8, 9] and (idx[2, 2:] == -1).all() and np.isinf(d2[2, 2:]).all()
    out = interpolate64(val[:10], idx, d2, 1e-8)
    w = 1.0 / (d2[:2, 3].astype(np.float64) + np.float64(np.float32(1e-8)))
    assert np.allclose(out[3], (w[:, None] * val[idx[:2, 3]]).sum(0) / w.sum(), rtol=1e-14)
