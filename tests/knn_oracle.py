"""numpy restatement of hpl_knn_interp (include/hpl_bcl.h): the search in float32 with the library's own
operations and order, so its neighbours and squared distances are the kernel's bit for bit; the interpolation in float64
from those float32 distances, which is what the kernel's float32 result is measured against.

Inputs are finite.  A d2 that overflows to +inf is not below the initial +inf and never enters (idx = -1), as in the kernel; a
query left without any neighbour interpolates to NaN (0 / 0) in both."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

INF_BITS = np.uint64(0x7f800000)


def _search_chunk(ref, q, k):
    """ref (3, N), q (3, n) float32 -> idx (k, n) int32, d2 (k, n) float32 of one pair."""
    N, n = ref.shape[1], q.shape[1]
    dx = q[0][:, None] - ref[0][None, :]                 # float32 arrays: every operation rounds to float32
    dy = q[1][:, None] - ref[1][None, :]
    dz = q[2][:, None] - ref[2][None, :]
    d2 = (dx * dx + dy * dy) + dz * dz
    # d2 >= +0, so its bit pattern orders like the value; bits << 32 | index orders by (d2, index): the strictly-smaller rule
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(N, dtype=np.uint64)[None, :]
    kk = min(k, N)
    if kk < N:
        key = np.partition(key, kk - 1, axis=1)[:, :kk]
    key = np.sort(key, axis=1)
    idx = np.full((k, n), -1, np.int32)
    out = np.full((k, n), np.inf, np.float32)
    found = (key >> np.uint64(32)) < INF_BITS
    idx[:kk] = np.where(found, (key & np.uint64(0xffffffff)).astype(np.int64), -1).T
    out[:kk] = np.where(found, (key >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf)).T
    return idx, out


def knn_search(ref, q, k, ref_prefix=None, q_prefix=None, chunk=1024, workers=8):
    """-> idx (k, Q) int32 into the packed ref, dist2 (k, Q) float32: ascending, ties to the smaller index, idx = -1 and
    dist2 = +inf where a pair has fewer than k points."""
    ref = np.ascontiguousarray(ref, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    assert np.isfinite(ref).all() and np.isfinite(q).all()
    N, Q = ref.shape[1], q.shape[1]
    rp = [0, N] if ref_prefix is None else list(ref_prefix)
    qp = [0, Q] if q_prefix is None else list(q_prefix)
    idx = np.full((k, Q), -1, np.int32)
    d2 = np.full((k, Q), np.inf, np.float32)

    def job(args):
        b, s, e = args
        i, d = _search_chunk(ref[:, rp[b]:rp[b + 1]], q[:, s:e], k)
        idx[:, s:e] = np.where(i >= 0, i + rp[b], -1)
        d2[:, s:e] = d
    jobs = [(b, s, min(qp[b + 1], s + chunk)) for b in range(len(rp) - 1) if rp[b + 1] > rp[b]
            for s in range(qp[b], qp[b + 1], chunk)]
    if len(jobs) > 1 and workers > 1:
        with ThreadPoolExecutor(workers) as ex:
            list(ex.map(job, jobs))
    else:
        for j in jobs:
            job(j)
    return idx, d2


def interpolate64(values, idx, d2, eps):
    """float64 evaluation of the library's weights from ITS float32 d2: sum w_i v_i / sum w_i with w_i = 1 / (d2_i + eps); a
    nearest d2 of exactly 0 takes that point's row.  -> [Q, C] float64."""
    v = np.asarray(values, np.float64)
    ok = idx >= 0
    with np.errstate(divide='ignore'):
        w = np.where(ok, 1.0 / (d2.astype(np.float64) + np.float64(np.float32(eps))), 0.0)      # (k, Q)
    rows = v[np.where(ok, idx, 0)]                                                              # (k, Q, C)
    with np.errstate(invalid='ignore'):
        out = (w[:, :, None] * rows).sum(0) / w.sum(0)[:, None]
    hit = d2[0] == 0
    out[hit] = v[idx[0][hit]]
    return out


def brute_force64(ref, q, k):
    """The k smallest squared distances in float64, ascending: (k, Q)."""
    r = np.asarray(ref, np.float64)
    p = np.asarray(q, np.float64)
    d2 = ((p[:, :, None] - r[:, None, :]) ** 2).sum(0)
    return np.sort(d2, axis=1)[:, :k].T
