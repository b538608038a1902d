"""numpy restatement of hpl_voxel_downsample (include/hpl_bcl.h), both modes: the cells by the float64 formula,
the voxels by a lexicographic sort of the signed cells, every sum in float64 one member after the other in ascending index from
0, one division, one rounding to float32, the nearest member in float32 with ties to the smaller index.  Every output is meant
to equal the library's bit for bit.  Also the scene generator of the voxel tests: ground_oracle.scene at lidar ranges."""
import numpy as np

import ground_oracle as G

CELL_MAX = 2 ** 18 - 2
MODES = {'centroid': 0, 'nearest': 1}
SHORT = 32                   # a run up to here is summed member by member across all voxels at once, a longer one on its own


def scene(n, seed, extent=60.0, **kw):
    """A cloud (3, n) float32: ground sheet, clutter and (wall=...) a wall over +-extent metres (ground_oracle.scene)."""
    return G.scene(n, seed, extent=extent, **kw)[0]


def cells(pc, voxel, origin=(0, 0, 0)):
    """-> (cell (3, n) float64, finite (n,), valid (n,)) of a cloud pc (3, n) float32."""
    inv = np.float64(1.0) / np.float64(np.float32(voxel))
    org = np.asarray(origin, np.float32).astype(np.float64)
    fin = np.isfinite(pc).all(0)
    with np.errstate(all='ignore'):
        c = np.floor((pc.astype(np.float64) - org[:, None]) * inv)
        valid = fin & (np.abs(c) <= CELL_MAX).all(0)
    return c, fin, valid


def _ordered_sums(rows, starts, lens):
    """rows (R, m) float64 in run order; -> (R, V) the sum of every run from 0, one member after the other."""
    out = np.zeros((rows.shape[0], len(starts)))
    with np.errstate(all='ignore'):
        for e in range(int(min(lens.max(initial=0), SHORT))):
            on = (lens > e) & (lens <= SHORT)
            out[:, on] = out[:, on] + rows[:, starts[on] + e]
        for v in np.flatnonzero(lens > SHORT):
            run = rows[:, starts[v]:starts[v] + lens[v]]
            out[:, v] = np.cumsum(np.concatenate([np.zeros((rows.shape[0], 1)), run], axis=1), axis=1)[:, -1]
    return out


def downsample_cloud(pc, attr=None, voxel=0.1, origin=(0, 0, 0), mode='centroid'):
    """One cloud pc (3, n) float32, attr (C, n) float32 or None.  -> dict(out_pc (3, n), out_attr (C, n) or None, count (n,),
    rep (n,), voxel_of (n,), stats (4,)) with indices and voxel positions relative to the cloud."""
    mode = MODES.get(mode, mode)
    n = pc.shape[1]
    C = 0 if attr is None else attr.shape[0]
    c, fin, valid = cells(pc, voxel, origin)
    out_pc, out_attr = np.zeros((3, n), np.float32), (np.zeros((C, n), np.float32) if C else None)
    count, rep, voxel_of = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    idx = np.flatnonzero(valid)
    cv = c[:, idx].astype(np.int64)
    order = idx[np.lexsort((cv[2], cv[1], cv[0]))]              # stable: ascending index inside a cell
    V = 0
    if len(order):
        cs = c[:, order]
        head = np.ones(len(order), bool)
        head[1:] = (cs[:, 1:] != cs[:, :-1]).any(0)
        starts = np.flatnonzero(head)
        V = len(starts)
        lens = np.diff(np.append(starts, len(order)))
        run_of = np.cumsum(head) - 1
        with np.errstate(all='ignore'):
            cen = (_ordered_sums(pc[:, order].astype(np.float64), starts, lens) / lens.astype(np.float64)).astype(np.float32)
            d = pc[:, order] - cen[:, run_of]                   # float32, every operation rounded
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            assert d2.dtype == np.float32
        best = np.minimum.reduceat(d2, starts)
        at = np.flatnonzero(d2 == best[run_of])                 # in run order, members in index order: the first one wins
        _, first = np.unique(run_of[at], return_index=True)
        r = order[at[first]]
        assert len(r) == V
        count[:V], rep[:V], voxel_of[order] = lens, r, run_of
        out_pc[:, :V] = pc[:, r] if mode else cen
        if C:
            if mode:
                out_attr[:, :V] = attr[:, r]
            else:
                with np.errstate(all='ignore'):
                    out_attr[:, :V] = (_ordered_sums(attr[:, order].astype(np.float64), starts, lens) /
                                       lens.astype(np.float64)).astype(np.float32)
    stats = np.array([V, len(idx), n - int(fin.sum()), int(fin.sum()) - len(idx)], np.int32)
    return dict(out_pc=out_pc, out_attr=out_attr, count=count, rep=rep, voxel_of=voxel_of, stats=stats)


def downsample(pc, attr=None, voxel=0.1, origin=(0, 0, 0), mode='centroid', prefix=None):
    """ops.voxel_downsample's outputs for a packed batch: dict(out_pc (3, N), out_attr (C, N) or None, count, rep, voxel_of
    (N,) int32 -- packed indices and positions --, stats (B, 4) int32)."""
    N = pc.shape[1]
    prefix = [0, N] if prefix is None else list(prefix)
    C = 0 if attr is None else attr.shape[0]
    o = dict(out_pc=np.zeros((3, N), np.float32), out_attr=np.zeros((C, N), np.float32) if C else None,
             count=np.zeros(N, np.int32), rep=np.full(N, -1, np.int32), voxel_of=np.full(N, -1, np.int32),
             stats=np.zeros((len(prefix) - 1, 4), np.int32))
    for b in range(len(prefix) - 1):
        p0, p1 = prefix[b], prefix[b + 1]
        w = downsample_cloud(pc[:, p0:p1], attr[:, p0:p1] if C else None, voxel, origin, mode)
        o['out_pc'][:, p0:p1], o['count'][p0:p1], o['stats'][b] = w['out_pc'], w['count'], w['stats']
        if C:
            o['out_attr'][:, p0:p1] = w['out_attr']
        o['rep'][p0:p1] = np.where(w['rep'] >= 0, w['rep'] + p0, -1)
        o['voxel_of'][p0:p1] = np.where(w['voxel_of'] >= 0, w['voxel_of'] + p0, -1)
    return o
