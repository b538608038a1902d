"""numpy restatement of hpl_fps (include/hpl_bcl.h): farthest point sampling over all points of a cloud, no grid,
no tricks.  Every float32 operation is one numpy float32 operation, so the device result is compared bit for bit."""
import numpy as np

F32 = np.float32


def d2_to(pc, s):
    """float32 (dx*dx + dy*dy) + dz*dz of every point of pc (3, n) to its point s."""
    with np.errstate(over='ignore', invalid='ignore'):
        dx, dy, dz = (pc[k] - pc[k, s] for k in range(3))
        return (dx * dx + dy * dy) + dz * dz


def sample_cloud(pc, m, attr=None, start=None):
    """One cloud: pc (3, n) float32, attr (C, n) float32 or None, start a cloud-local index or None.
    -> dict(idx (m,), dist (m,), out_pc (3, m), out_attr (C, m) or None, cover (n,), count, valid, nonfinite)."""
    pc = np.ascontiguousarray(pc, dtype=F32)
    n = pc.shape[1]
    ok = np.isfinite(pc).all(axis=0)
    idx, dist = np.full(m, -1, np.int32), np.zeros(m, F32)
    D = np.where(ok, F32(np.inf), F32(-1))                    # -1: never selected, never counted
    count = 0
    if ok.any():
        s = int(start) if start is not None and n > 0 and ok[int(start)] else int(np.flatnonzero(ok)[0])
        idx[0], dist[0], count = s, np.inf, 1
        while True:
            D = np.where(ok, np.minimum(D, np.where(ok, d2_to(pc, s), F32(0))), D)
            s = int(np.argmax(D))                             # (the first of the largest: ties to the smaller index)
            if count == m or D[s] == 0:
                break
            idx[count], dist[count] = s, D[s]
            count += 1
    sel = idx[:count]
    out_pc = np.zeros((3, m), F32)
    out_pc[:, :count] = pc[:, sel]
    out_attr = None
    if attr is not None:
        out_attr = np.zeros((attr.shape[0], m), F32)
        out_attr[:, :count] = attr[:, sel]
    return dict(idx=idx, dist=dist, out_pc=out_pc, out_attr=out_attr, cover=np.where(ok, D, F32(0)).astype(F32), count=count,
                valid=int(ok.sum()), nonfinite=int(n - ok.sum()))


def sample(pc, m, attr=None, start=None, prefix=None, path=0):
    """The packed ragged batch as hpl_fps returns it: idx / dist (B, m), out_pc (3, B m), out_attr (C, B m), cover (N,),
    stats (B, 4) = (count, valid, non-finite, path)."""
    N = pc.shape[1]
    prefix = [0, N] if prefix is None else list(prefix)
    B = len(prefix) - 1
    rows = [sample_cloud(pc[:, prefix[b]:prefix[b + 1]], m, None if attr is None else attr[:, prefix[b]:prefix[b + 1]],
                         None if start is None else start[b]) for b in range(B)]
    return dict(idx=np.stack([r['idx'] for r in rows]), dist=np.stack([r['dist'] for r in rows]),
                out_pc=np.concatenate([r['out_pc'] for r in rows], axis=1),
                out_attr=None if attr is None else np.concatenate([r['out_attr'] for r in rows], axis=1),
                cover=np.concatenate([r['cover'] for r in rows]) if rows else np.zeros(0, F32),
                stats=np.array([[r['count'], r['valid'], r['nonfinite'], path] for r in rows], np.int32).reshape(B, 4))


def cloud(n, seed, extent=10.0):
    """A seeded uniform cloud (3, n) float32."""
    return np.random.RandomState(seed).uniform(-extent, extent, (3, n)).astype(F32)


def grid(k=6):
    """The integer grid k x k x k in `ij` order: every round has ties."""
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing='ij')).reshape(3, -1)
    return g.astype(F32)
