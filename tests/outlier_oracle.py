"""numpy restatement of hpl_outlier_filter (include/hpl_bcl.h).  The neighbourhood is the interface's all-pairs
definition in exactly its float32 arithmetic, by brute force in chunks: there is no grid here.  A vectorised form and a plain
double loop state it twice.  The per-cloud sums are numpy's float64 sums, not the kernel's fixed order: the thresholds agree
to the rounding of those sums, everything per point agrees bit for bit."""
import numpy as np

from icp_oracle import in_range
from normals_oracle import scene as surface_scene

STATISTICAL, RADIUS = 'statistical', 'radius'


def _prefix(pc, prefix):
    return [0, pc.shape[1]] if prefix is None else [int(x) for x in prefix]


def neighbourhoods(pc, k, radius, prefix=None, chunk=256):
    """-> (total (N,) int32: the neighbours of every point, not capped; nbr_d2 (N, k) float32: the min(k, total) smallest d2
    ascending, then +inf).  The neighbours of a point that takes part: the OTHER indices of its cloud that take part with float32
    d2 = (dx * dx + dy * dy) + dz * dz <= float32(radius * radius) and d2 < +inf."""
    pc = np.asarray(pc, np.float32)
    N = pc.shape[1]
    prefix = _prefix(pc, prefix)
    rad = np.float32(radius)
    with np.errstate(over='ignore'):
        r2 = np.float32(rad * rad)
    total = np.zeros(N, np.int32)
    nd2 = np.full((N, k), np.inf, np.float32)
    part = in_range(pc, radius) if N else np.zeros(0, bool)
    for p0, p1 in zip(prefix, prefix[1:]):
        c = pc[:, p0:p1]
        J = np.arange(p0, p1)
        for lo in range(0, p1 - p0, chunk):
            q = c[:, lo:lo + chunk]
            I = J[lo:lo + chunk]
            with np.errstate(invalid='ignore', over='ignore'):
                dx = q[0][:, None] - c[0][None, :]
                dy = q[1][:, None] - c[1][None, :]
                dz = q[2][:, None] - c[2][None, :]
                d2 = (dx * dx + dy * dy) + dz * dz
                assert d2.dtype == np.float32
                acc = part[I, None] & part[None, p0:p1] & (d2 <= r2) & (d2 < np.float32(np.inf)) & (I[:, None] != J[None, :])
            vals = np.where(acc, d2, np.float32(np.inf))
            if k < vals.shape[1]:                             # the k smallest values, whichever way they are found
                vals = np.partition(vals, k - 1, axis=1)[:, :k]
            vals = np.sort(vals, axis=1)
            total[I] = acc.sum(1)
            nd2[I, :vals.shape[1]] = vals
    return total, nd2


def neighbourhoods_loop(pc, k, radius, prefix=None):
    """neighbourhoods() as a plain double loop over the pairs of a cloud."""
    pc = np.asarray(pc, np.float32)
    N = pc.shape[1]
    prefix = _prefix(pc, prefix)
    rad = np.float32(radius)
    with np.errstate(over='ignore'):
        r2 = np.float32(rad * rad)
    inv_cell = 1.0 / (1.001 * np.float64(rad))
    total = np.zeros(N, np.int32)
    nd2 = np.full((N, k), np.inf, np.float32)

    def takes_part(j):
        p = pc[:, j].astype(np.float64)
        if not np.isfinite(p).all():
            return False
        return bool((np.abs(np.floor(p * inv_cell)) <= 2 ** 18 - 2).all())

    part = [takes_part(j) for j in range(N)]
    for p0, p1 in zip(prefix, prefix[1:]):
        for i in range(p0, p1):
            if not part[i]:
                continue
            found = []
            for j in range(p0, p1):
                if j == i or not part[j]:
                    continue
                with np.errstate(over='ignore'):
                    dx, dy, dz = pc[0, i] - pc[0, j], pc[1, i] - pc[1, j], pc[2, i] - pc[2, j]
                    d2 = np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))
                if d2 <= r2 and d2 < np.float32(np.inf):
                    found.append(d2)
            found.sort()
            total[i] = len(found)
            nd2[i, :min(k, len(found))] = found[:k]
    return total, nd2


def mean_distance(nd2, total, k, radius, part):
    """-> (mean_dist (N,) float32, count (N,) int32): S = the float64 sum of the roots in list order from 0, a missing neighbour
    at the radius, divided by k and rounded once; +inf and 0 where the point takes no part."""
    count = np.minimum(total, k).astype(np.int32)
    S = np.zeros(len(total))
    for t in range(k):
        on = t < count
        S = np.where(on, S + np.sqrt(np.where(on, nd2[:, t], 0).astype(np.float64)), S)
    s = S + (k - count).astype(np.float64) * np.float64(np.float32(radius))
    m = (s / np.float64(k)).astype(np.float32)
    return np.where(part, m, np.float32(np.inf)), np.where(part, count, 0).astype(np.int32)


def thresholds(mean_dist, part, prefix, std_ratio):
    """-> (B, 3) float64 (mu, sigma, T) per cloud, from the float32 mean_dist widened: two passes, the sample form."""
    out = np.zeros((len(prefix) - 1, 3))
    for b, (p0, p1) in enumerate(zip(prefix, prefix[1:])):
        m = mean_dist[p0:p1][part[p0:p1]].astype(np.float64)
        n = len(m)
        mu = m.sum() / n if n else 0.0
        sigma = np.sqrt(((m - mu) ** 2).sum() / (n - 1)) if n >= 2 else 0.0
        out[b] = mu, sigma, mu + np.float64(np.float32(std_ratio)) * sigma
    return out


def classify(part, prefix, mode, mean_dist=None, thresh=None, count=None, min_neighbors=None):
    """-> (keep (N,) uint8, keep_idx (N,) int32, stats (B, 4) int32) from published values: statistical: the float32 mean_dist
    against the float32 thresh[b][2]; radius: count against min_neighbors."""
    N = len(part)
    B = len(prefix) - 1
    keep = np.zeros(N, np.uint8)
    keep_idx = np.full(N, -1, np.int32)
    stats = np.zeros((B, 4), np.int32)
    for b, (p0, p1) in enumerate(zip(prefix, prefix[1:])):
        p = part[p0:p1]
        if mode == STATISTICAL:
            k = p & (np.asarray(mean_dist, np.float32)[p0:p1] <= np.float32(thresh[b][2]))
        else:
            k = p & (count[p0:p1] >= min_neighbors)
        keep[p0:p1] = k
        idx = p0 + np.nonzero(k)[0]
        keep_idx[p0:p0 + len(idx)] = idx
        stats[b] = p.sum(), k.sum(), p.sum() - k.sum(), (p1 - p0) - p.sum()
    return keep, keep_idx, stats


def outlier_filter(pc, mode=STATISTICAL, k=16, radius=1.0, std_ratio=2.0, min_neighbors=None, prefix=None, loop=False, chunk=256):
    """-> dict(keep, keep_idx, mean_dist (None in radius mode), count, nbr_d2 (None in radius mode), thresh (B, 4) float32,
    thresh64 (B, 3) float64, stats, part)."""
    pc = np.asarray(pc, np.float32)
    prefix = _prefix(pc, prefix)
    part = in_range(pc, radius) if pc.shape[1] else np.zeros(0, bool)
    B = len(prefix) - 1
    kk = k if mode == STATISTICAL else 1
    total, nd2 = neighbourhoods_loop(pc, kk, radius, prefix) if loop else neighbourhoods(pc, kk, radius, prefix, chunk)
    if mode == STATISTICAL:
        mean_dist, count = mean_distance(nd2, total, k, radius, part)
        t64 = thresholds(mean_dist, part, prefix, std_ratio)
        thresh = np.zeros((B, 4), np.float32)
        thresh[:, :3] = t64.astype(np.float32)
        keep, keep_idx, stats = classify(part, prefix, mode, mean_dist=mean_dist, thresh=thresh)
        nd2 = np.where(np.arange(k)[None, :] < count[:, None], nd2, np.float32(np.inf))
    else:
        mean_dist, nd2, count = None, None, np.where(part, total, 0).astype(np.int32)
        t64, thresh = np.zeros((B, 3)), np.zeros((B, 4), np.float32)
        keep, keep_idx, stats = classify(part, prefix, mode, count=count, min_neighbors=min_neighbors)
    return dict(keep=keep, keep_idx=keep_idx, mean_dist=mean_dist, count=count, nbr_d2=nd2, thresh=thresh, thresh64=t64,
                stats=stats, part=part)


def scene(n, n_out, seed):
    """-> (pc (3, n) float32, stray (n,) bool): normals_oracle.scene(n - n_out, seed) and n_out strays drawn uniformly in
    x in [-8, 8], y in [4.5, 9], z in [2, 18] -- above every surface of that scene --, the columns permuted."""
    surf = surface_scene(n - n_out, seed)
    rng = np.random.RandomState(1000 + seed)
    strays = np.stack([rng.uniform(-8, 8, n_out), rng.uniform(4.5, 9, n_out), rng.uniform(2, 18, n_out)]).astype(np.float32)
    perm = rng.permutation(n)
    pc = np.concatenate([surf, strays], 1)[:, perm]
    return np.ascontiguousarray(pc), (perm >= n - n_out)
