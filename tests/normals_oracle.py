"""numpy restatement of hpl_normals (include/hpl_bcl.h).  The neighbourhood is the interface's all-pairs
definition in exactly its float32 arithmetic, by brute force: there is no grid here.  The covariance is the interface's float64
sums in neighbourhood order; the eigenpair comes by a different method from the kernel's: np.linalg.eigh where the kernel runs
cyclic Jacobi sweeps."""
import numpy as np

from icp_oracle import in_range


def neighbourhoods(pc, k, radius, prefix=None, chunk=256):
    """-> (count (N,) int32, nbr (N, k) int32 then -1, nbr_d2 (N, k) float32 then +inf) of the packed clouds pc (3, N): per point
    that takes part the points of its cloud that take part with float32 d2 = (dx * dx + dy * dy) + dz * dz <=
    float32(radius * radius), ordered by (d2, index), the first k."""
    pc = np.asarray(pc, np.float32)
    N = pc.shape[1]
    prefix = [0, N] if prefix is None else [int(x) for x in prefix]
    rad = np.float32(radius)
    r2 = np.float32(rad * rad)
    count = np.zeros(N, np.int32)
    nbr = np.full((N, k), -1, np.int32)
    nd2 = np.full((N, k), np.inf, np.float32)
    part = in_range(pc, radius) if N else np.zeros(0, bool)
    for p0, p1 in zip(prefix, prefix[1:]):
        c = pc[:, p0:p1]
        J = np.arange(p0, p1)
        for lo in range(0, p1 - p0, chunk):
            q = c[:, lo:lo + chunk]
            with np.errstate(invalid='ignore', over='ignore'):
                dx = q[0][:, None] - c[0][None, :]
                dy = q[1][:, None] - c[1][None, :]
                dz = q[2][:, None] - c[2][None, :]
                d2 = (dx * dx + dy * dy) + dz * dz
                assert d2.dtype == np.float32
                acc = part[p0 + lo:p0 + lo + q.shape[1], None] & part[None, p0:p1] & (d2 <= r2)
            Jb = np.broadcast_to(J[None, :], d2.shape)
            rows = np.arange(q.shape[1])[:, None]
            # (acceptable, d2, index) ascending: the columns stand in index order and both sorts are stable
            by_d2 = np.argsort(np.where(acc, d2, np.float32(np.inf)), axis=1, kind='stable')
            order = by_d2[rows, np.argsort(~acc[rows, by_d2], axis=1, kind='stable')][:, :k]
            ok = acc[rows, order]
            w = order.shape[1]
            sl = slice(p0 + lo, p0 + lo + q.shape[1])
            count[sl] = ok.sum(1)
            nbr[sl, :w] = np.where(ok, Jb[rows, order], -1)
            nd2[sl, :w] = np.where(ok, d2[rows, order], np.float32(np.inf))
    return count, nbr, nd2


def covariance(pc, count, nbr):
    """-> (m (N, 3), C (N, 3, 3)) float64: the mean and the scatter sums of each neighbourhood, every sum in list order from 0."""
    p = np.asarray(pc, np.float32).astype(np.float64)
    N, k = nbr.shape
    m = np.zeros((N, 3))
    for t in range(k):
        on = (t < count)[:, None]
        m = np.where(on, m + p[:, np.where(nbr[:, t] >= 0, nbr[:, t], 0)].T, m)
    with np.errstate(invalid='ignore', divide='ignore'):
        m = m / count[:, None].astype(np.float64)
    C = np.zeros((N, 3, 3))
    for t in range(k):
        on = (t < count)[:, None, None]
        d = p[:, np.where(nbr[:, t] >= 0, nbr[:, t], 0)].T - m
        C = np.where(on, C + d[:, :, None] * d[:, None, :], C)
    return m, C


def normals(pc, k=16, radius=1.0, viewpoint=None, prefix=None):
    """-> dict(normal (3, N) float32, curvature (N,) float32, count, nbr, nbr_d2, valid (N,) bool, lam (N, 3) float64 ascending,
    gap (N,) = (lam1 - lam0) / lam2 (0 where invalid), n64 (3, N) the float64 unit normal).  viewpoint: None, three numbers or
    one triple per cloud."""
    pc = np.asarray(pc, np.float32)
    N = pc.shape[1]
    prefix = [0, N] if prefix is None else [int(x) for x in prefix]
    B = len(prefix) - 1
    count, nbr, nd2 = neighbourhoods(pc, k, radius, prefix)
    _, C = covariance(pc, count, nbr)
    finite = np.isfinite(C).all((1, 2)) & (count >= 3)
    lam, vec = np.linalg.eigh(np.where(finite[:, None, None], C, np.eye(3)[None]))
    n = vec[:, :, 0]
    n = n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
    valid = finite & np.isfinite(lam).all(1) & (lam[:, 2] > 0)
    view = np.zeros((B, 3), np.float32) if viewpoint is None else np.asarray(viewpoint, np.float32).reshape(-1, 3)
    view = np.broadcast_to(view, (B, 3)).astype(np.float64)
    v = np.repeat(view, np.diff(prefix), axis=0)
    with np.errstate(invalid='ignore', over='ignore'):
        e = v - pc.T.astype(np.float64)
        s = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
    lead = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
    flip = (s < 0) | ((s == 0) & (lead < 0))
    n = np.where(flip[:, None], -n, n)
    with np.errstate(invalid='ignore', divide='ignore'):
        curv = np.maximum(lam[:, 0], 0) / ((lam[:, 0] + lam[:, 1]) + lam[:, 2])
        gap = np.where(valid, (lam[:, 1] - lam[:, 0]) / lam[:, 2], 0.0)
    n = np.where(valid[:, None], n, 0.0)
    return dict(normal=n.T.astype(np.float32), curvature=np.where(valid, curv, 0.0).astype(np.float32), count=count, nbr=nbr,
                nbr_d2=nd2, valid=valid, lam=lam, gap=gap, n64=n.T)


def scene(n, seed, sigma=0.01):
    """Surfaces sampled at random -> (3, n) float32: the ground y = -1.5 over [-8, 8] x [2, 18] (n / 2 points), the walls x = -8
    and z = 18, 4 m high (n / 5 each), the upper half of a sphere of radius 2 about (2, -1.5, 9) (the rest); N(0, sigma) noise
    on every coordinate; the columns permuted."""
    rng = np.random.RandomState(seed)
    ng, nw = n // 2, n // 5
    ns = n - ng - 2 * nw
    ground = np.stack([rng.uniform(-8, 8, ng), np.full(ng, -1.5), rng.uniform(2, 18, ng)])
    wall_x = np.stack([np.full(nw, -8.0), rng.uniform(-1.5, 2.5, nw), rng.uniform(2, 18, nw)])
    wall_z = np.stack([rng.uniform(-8, 8, nw), rng.uniform(-1.5, 2.5, nw), np.full(nw, 18.0)])
    d = rng.normal(0, 1, (3, ns))
    d = d / np.linalg.norm(d, axis=0)
    d[1] = np.abs(d[1])
    sphere = np.array([[2.0], [-1.5], [9.0]]) + 2.0 * d
    p = np.concatenate([ground, wall_x, wall_z, sphere], 1) + rng.normal(0, sigma, (3, n))
    return p[:, rng.permutation(n)].astype(np.float32)
