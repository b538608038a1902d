"""CPU: the engine's --dense rules, the dense-flow ABI entries in include/hpl_bcl.h and their ctypes mirror, and the numpy
restatement the GPU tests use for hpl_lattice_query (tests/dense_oracle.py) against the C oracle's generate_data for queries
equal to pc1."""
import ctypes
import os
import re

import numpy as np
import pytest

from common import ROOT
from hplflownet_amd import _lib
from hplflownet_amd.synthetic import synthetic_pair


def header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read(), flags=re.S)


def test_header_declares_the_query_entries():
    h = header()
    for name in ('hpl_lattice_query_info', 'hpl_lattice_query'):
        assert re.search(r'\b%s\s*\(' % name, h), name
        assert name in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, 'hpl_lattice_query') and hasattr(lib, 'hpl_lattice_query_info')


def test_query_info_layout_matches_header():
    h = header()
    struct = h[h.index('typedef struct hpl_query_info {'):h.index('} hpl_query_info;')]
    names = re.findall(r'(\w+)\s*[;,]', struct.split('{', 1)[1])
    assert names == [f[0] for f in _lib.QueryInfo._fields_]
    assert ctypes.sizeof(_lib.QueryInfo) == 64


def test_query_refuses_bad_arguments_without_a_launch():
    lib = _lib.load()
    info = _lib.QueryInfo()
    pre = (ctypes.c_int64 * 2)(0, 5)
    # no table in the info, Q out of range, null pointers: HPL_EINVAL before anything touches a device
    assert lib.hpl_lattice_query(ctypes.byref(info), 256, 5, pre, 1, 256, 256, 256, None) == -1
    info.slots, info.mm, info.H0, info.batch = 256, 256, 1, 1
    assert lib.hpl_lattice_query(ctypes.byref(info), 256, 0, None, 1, 256, 256, 256, None) == -1
    assert lib.hpl_lattice_query(ctypes.byref(info), None, 5, None, 1, 256, 256, 256, None) == -1
    assert lib.hpl_lattice_query(ctypes.byref(info), 256, 5, (ctypes.c_int64 * 2)(0, 4), 1, 256, 256, 256, None) == -1
    info.batch = 2
    assert lib.hpl_lattice_query(ctypes.byref(info), 256, 5, None, 1, 256, 256, 256, None) == -1
    assert lib.hpl_lattice_query_info(None, ctypes.byref(info)) == -1


def test_numpy_restatement_on_pc1_points():
    from dense_oracle import NpQuery
    from oracle import lattice_oracle as LO
    from hplflownet_amd.synthetic import SCALES_FILTER_MAP
    a, b, _ = synthetic_pair(512, 4)
    p1, p2 = a.T.copy(), b.T.copy()
    gd = LO.generate_data(p1.T, p2.T, SCALES_FILTER_MAP[:1])[0]
    for renorm in (False, True):
        off, bary, cov, aliased = NpQuery(p1, p2)(p1, renorm)
        assert np.array_equal(off, gd['pc1_lattice_offset'])
        assert np.array_equal(bary.view(np.int32), gd['pc1_barycentric'].astype(np.float32).view(np.int32))
        assert (cov == 1).all() and not aliased.any()


def test_dense_argparse_rules(tmp_path):
    from hplflownet_amd import engine
    root = str(tmp_path)
    a = engine.parse_args(['--evaluate', '--dense', '--dataset', 'FlyingThings3DSubset', '--data-root', root])
    assert a.dense
    a = engine.parse_args(['--evaluate', '--dense', '--dataset', 'KITTI', '--data-root', root, '--batch-size', '2', '--ragged'])
    assert a.dense and a.ragged and a.batch_size == 2
    assert not engine.parse_args(['--evaluate', '--dataset', 'KITTI', '--data-root', root]).dense
    for bad in (['--dense'], ['--evaluate', '--dense'], ['--dense', '--dataset', 'FlyingThings3DSubset', '--data-root', root],
                ['--evaluate', '--dense', '--dataset', 'synthetic']):
        with pytest.raises(SystemExit):
            engine.parse_args(bad)
