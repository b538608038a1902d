#!/usr/bin/env python
"""GPU: dense scene flow (flownet.DenseFlow) on synthetic frustum frames of M points, 8 192 of them sampled per
cloud -- one table for profiles/dense_flow_bench.txt.

Per M in --sizes (HPLFlowNet, hash init, eval mode, no grad), all times from device events, medians of --reps after warm-up:
  forward   model(pc1, pc2, lat) (the native plan) against DenseFlow.forward (the pair-batched Python path keeping Z);
  lookup    hpl_lattice_query of the frame's M pc1 points;
  slice     hpl_slice of Z at those points (the head's first step, alone);
  query     DenseFlow.query of the M points (lookup + slice + trailing 1x1 + conv2 / conv3 / conv4), and head = query - lookup
            - slice;
  coverage  mean coverage and the fraction of fully covered queries;
  fill      (profiles/dense_fill_bench.txt) hpl_knn_interp at k = --k over the M queries in the coverage form
            query(fill='knn') uses (fully covered lanes idle), beside the plain form over all M queries (no lane idle) and
            over the uncovered queries only, selected beforehand (what compacting them first could reach, its select and
            scatter not counted); query_fill = DenseFlow.query(fill='knn') whole.
--lookup-only / --fill-only: only hpl_lattice_query / only the coverage-form hpl_knn_interp, --reps times per size (what
`rocprofv3 --kernel-trace --stats` is run on)."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='65536,262144,450000')
    ap.add_argument('--points', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--lookup-only', action='store_true')
    ap.add_argument('--fill-only', action='store_true')
    ap.add_argument('--k', type=int, default=3)
    a = ap.parse_args()
    import hplflownet_amd as H
    from hplflownet_amd import ops
    from hplflownet_amd.synthetic import SCALES_FILTER_MAP, fill_module_, synthetic_pair
    dev = torch.device('cuda:0')
    args = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP, evaluate=True, use_leaky=True, bcn_use_bias=True,
                                 bcn_use_norm=True, last_relu=False, DEVICE='cuda')
    m = H.HPLFlowNet(args)
    fill_module_(m, 1.0, 'hash')
    m = m.to(dev).eval()
    gen = H.GenerateDataUnsymmetric(args, device=dev, wide_up=m.lattice_hint())
    df = H.DenseFlow(m)
    rows = []
    with torch.no_grad():
        for M in [int(x) for x in a.sizes.split(',')]:
            f1, f2, _ = synthetic_pair(M, 7)
            rng = np.random.RandomState(0)
            s1, s2 = rng.choice(M, a.points, replace=False), rng.choice(M, a.points, replace=False)
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x.T, dtype=np.float32)).to(dev)       # noqa: E731
            p1, p2, q = t(f1[s1]), t(f2[s2]), t(f1)
            lat = gen.build_native(p1, p2)
            for _ in range(3):
                flow, state = df.forward(p1[None], p2[None], lat)
            cov = torch.empty(M, dtype=torch.float32, device=dev)
            lookup = timed(lambda: df.locate(state, q, [0, M], True, cov), a.reps)
            if a.lookup_only:
                rows.append(dict(M=M, lookup_ms=lookup))
                continue
            if a.fill_only:
                base, _ = df.query(state, q)
                base = base.t().contiguous()
                spc, sfl, _ = state.fill_inputs()
                fill = timed(lambda: ops.knn_interpolate(spc, sfl, q, k=a.k, out=base, coverage=cov), a.reps)
                rows.append(dict(M=M, k=a.k, fill_ms=fill))
                continue
            fwd_model = timed(lambda: m(p1[None], p2[None], lat), a.reps)
            fwd_dense = timed(lambda: df.forward(p1[None], p2[None], lat), a.reps)
            bary, off = df.locate(state, q, [0, M], True, cov)
            C = state.Z.shape[1]

            def slice_all():
                for s in range(0, M, df.CHUNK):
                    e = min(M, s + df.CHUNK)
                    ops.slice_raw(state.Z, bary[:, s:e].contiguous(), off[:, s:e].contiguous(), e - s)
            df.query(state, q)
            sl = timed(slice_all, a.reps)
            qt = timed(lambda: df.query(state, q), a.reps)
            qb, c = df.query(state, q)
            base = qb.t().contiguous()
            spc, sfl, _ = state.fill_inputs()
            fill = timed(lambda: ops.knn_interpolate(spc, sfl, q, k=a.k, out=base, coverage=c), a.reps)
            fill_all = timed(lambda: ops.knn_interpolate(spc, sfl, q, k=a.k), a.reps)
            qu = q[:, c != 1].contiguous()
            fill_sel = timed(lambda: ops.knn_interpolate(spc, sfl, qu, k=a.k), a.reps)
            df.query(state, q, fill='knn', k=a.k)
            qft = timed(lambda: df.query(state, q, fill='knn', k=a.k), a.reps)
            rows.append(dict(M=M, sampled=a.points, H0=int(state.Z.shape[0]), Z_cols=C, forward_model_ms=fwd_model,
                             forward_dense_ms=fwd_dense, lookup_ms=lookup, slice_ms=sl, query_ms=qt,
                             head_ms=qt - lookup - sl, k=a.k, fill_ms=fill, fill_all_queries_ms=fill_all,
                             fill_uncovered_only_ms=fill_sel, query_fill_ms=qft, coverage=float(c.double().mean()), full=float((c == 1).double().mean())))
            print(json.dumps(rows[-1]), flush=True)
    if a.lookup_only or a.fill_only:
        print(json.dumps(rows))


if __name__ == '__main__':
    main()
