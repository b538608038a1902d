"""numpy restatement of hpl_icp (include/hpl_bcl.h) for one pair.  The match is the interface's all-pairs
definition in exactly its float32 arithmetic, by brute force: there is no grid here.  The round's solve comes by a different
method from the kernel's: a float64 SVD (Kabsch, rigid_oracle.kabsch) where the kernel takes Horn's quaternion.  `dtype` is
the precision of the residuals, the weights, the centroids and the covariance: float64 is the reference, float32 shows what a
float32 round over the same matches would lose (the bars of tests/test_gpu_icp.py come from the difference)."""
import numpy as np

from rigid_oracle import kabsch, rotation

CELL_MARGIN = 1.001
CELL_MAX = 2 ** 18 - 2

IDENTITY = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32))


def in_range(x, max_dist):
    """(n,) bool: the points of x (3, n) float32 that are finite and whose cells fit the key's fields."""
    inv_cell = 1.0 / (CELL_MARGIN * np.float64(np.float32(max_dist)))
    with np.errstate(invalid='ignore', over='ignore'):
        c = np.floor(np.asarray(x, np.float32).astype(np.float64) * inv_cell)
        return (np.abs(c) <= CELL_MAX).all(0)            # (NaN and inf fail)


def moved(p, R, t):
    """y (3, n) float64: y_k = ((R[k][0] px + R[k][1] py) + R[k][2] pz) + t_k from the float32 p, R, t, widened."""
    p = np.asarray(p, np.float32).astype(np.float64)
    R = np.asarray(R, np.float32).astype(np.float64)
    t = np.asarray(t, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([((R[k, 0] * p[0] + R[k, 1] * p[1]) + R[k, 2] * p[2]) + t[k] for k in range(3)])


def match(src, dst, R, t, max_dist, chunk=512):
    """The matches of src (3, n) under the float32 motion (R, t) among dst (3, m) -> (match (n,) int32 or -1, dist2 (n,) float32
    or +inf).  Vectorised all-pairs: float32 d2 = (dx * dx + dy * dy) + dz * dz, the smallest one, ties to the smaller index,
    accepted when d2 <= float32(max_dist * max_dist)."""
    src, dst = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    n, m = src.shape[1], dst.shape[1]
    idx = np.full(n, -1, np.int32)
    d2o = np.full(n, np.inf, np.float32)
    if n == 0 or m == 0:
        return idx, d2o
    md = np.float32(max_dist)
    md2 = np.float32(md * md)
    with np.errstate(invalid='ignore', over='ignore'):
        yq = moved(src, R, t).astype(np.float32)
    part = in_range(dst, max_dist)
    qok = in_range(yq, max_dist)
    for lo in range(0, n, chunk):
        q = yq[:, lo:lo + chunk]
        with np.errstate(invalid='ignore', over='ignore'):
            dx = q[0][:, None] - dst[0][None, :]
            dy = q[1][:, None] - dst[1][None, :]
            dz = q[2][:, None] - dst[2][None, :]
            d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        d2 = np.where(part[None, :] & ~np.isnan(d2), d2, np.float32(np.inf))
        j = d2.argmin(1)                                 # (the first of equal minima: the smaller index)
        best = d2[np.arange(d2.shape[0]), j]
        hit = (best <= md2) & qok[lo:lo + chunk]
        idx[lo:lo + chunk] = np.where(hit, j, -1)
        d2o[lo:lo + chunk] = np.where(hit, best, np.float32(np.inf))
    return idx, d2o


def base_weights(src, w):
    """The effective base weights (float64): w (or 1), 0 where w is not in (0, inf) or the point is not finite."""
    n = src.shape[1]
    w = np.ones(n, np.float32) if w is None else np.asarray(w, np.float32)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(src).all(0) & (w > 0) & np.isfinite(w)
    return np.where(ok, w, 0).astype(np.float64)


def residuals2(src, dst, idx, R, t, dtype=np.float64):
    """r2 (n,) in dtype against the matched points (0 where there is none)."""
    hit = idx >= 0
    if not hit.any():
        return np.zeros(len(idx), dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        y = moved(src, R, t).astype(dtype)
    q = np.asarray(dst, np.float32)[:, np.where(hit, idx, 0)].astype(dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        r2 = ((y - q) ** 2).sum(0, dtype=dtype)
    return np.where(hit, r2, 0).astype(dtype)


def round_(src, dst, R, t, w=None, max_dist=1.0, tau=0.3, dtype=np.float64, matched=None):
    """One round from the float32 motion (R, t) -> dict(ok, R (3, 3) float64, t (3,) float64, R32, t32 (what the round hands
    on: float32; the motion it started from when it failed), match, dist2).  matched: (match, dist2) of an earlier call with
    the same clouds, motion and max_dist (the match does not depend on dtype)."""
    src, dst = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    R0, t0 = np.asarray(R, np.float32), np.asarray(t, np.float32)
    n, m = src.shape[1], dst.shape[1]
    idx, d2 = match(src, dst, R0, t0, max_dist) if matched is None else matched
    fail = dict(ok=False, R=R0.astype(np.float64), t=t0.astype(np.float64), R32=R0, t32=t0, match=idx, dist2=d2)
    if n < 3 or m == 0:
        return fail
    w0 = base_weights(src, w).astype(dtype)
    live = (w0 > 0) & (idx >= 0)
    r2 = residuals2(src, dst, idx, R0, t0, dtype)
    tau = dtype(np.float32(tau))
    u = np.where(live, w0 / (1 + np.where(live, r2, 0) / (tau * tau)) ** 2, 0).astype(dtype)
    W = u.sum(dtype=dtype)
    if not (W > 0 and np.isfinite(W)):
        return fail
    P = np.where(live, src, 0).astype(dtype)
    Q = np.where(live, dst[:, np.where(idx >= 0, idx, 0)], 0).astype(dtype)
    mp, mq = (P * u).sum(1, dtype=dtype) / W, (Q * u).sum(1, dtype=dtype) / W
    H = ((P - mp[:, None]) * u) @ (Q - mq[:, None]).T
    Rn = kabsch(H)
    tn = mq.astype(np.float64) - Rn @ mp.astype(np.float64)
    if not (np.isfinite(Rn).all() and np.isfinite(tn).all()):
        return fail
    return dict(ok=True, R=Rn, t=tn, R32=Rn.astype(np.float32), t32=tn.astype(np.float32), match=idx, dist2=d2)


def angle_deg(R):
    """atan2(|v|, tr R - 1) in degrees, v the axial vector of R - R^T (twice the sine and twice the cosine)."""
    R = np.asarray(R, np.float64)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.degrees(np.arctan2(np.linalg.norm(v), np.trace(R) - 1.0)))


def finish(src, dst, R, t, w=None, max_dist=1.0, dtype=np.float64, matched=None):
    """The outputs of the finish under the float32 motion (R, t) -> dict(match, dist2, flow (n, 3) float64, share, rmse,
    angle_deg, trans).  matched: as round_ takes it."""
    src, dst = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    n = src.shape[1]
    idx, d2 = match(src, dst, R, t, max_dist) if matched is None else matched
    live = (base_weights(src, w) > 0) & (idx >= 0)
    r2 = residuals2(src, dst, idx, R, t, dtype)
    cnt = int(live.sum())
    with np.errstate(invalid='ignore', over='ignore'):
        flow = (moved(src, R, t) - src.astype(np.float64)).T
    return dict(match=idx, dist2=d2, flow=flow, share=cnt / max(n, 1),
                rmse=float(np.sqrt(r2[live].sum(dtype=dtype) / cnt)) if cnt else 0.0,
                angle_deg=angle_deg(np.asarray(R, np.float32)), trans=float(np.linalg.norm(np.asarray(t, np.float32).astype(np.float64))))


def chain(src, dst, init=None, iters=30, w=None, max_dist=1.0, tau=0.3, tol_rot=0.0, tol_trans=0.0, dtype=np.float64):
    """The chained driver: up to `iters` rounds, each from the previous round's float32 motion; stops at a failed round and
    after a round that moved no R entry by more than tol_rot and no t entry by more than tol_trans.
    -> dict(R32, t32, status, rounds, history [(R32, t32) after each round run])."""
    src = np.asarray(src, np.float32)
    R, t = (np.asarray(x, np.float32) for x in (IDENTITY if init is None else init))
    status = int(src.shape[1] >= 3 and np.asarray(dst).shape[1] > 0)
    rounds, hist = 0, []
    while status and rounds < iters:
        r = round_(src, dst, R, t, w, max_dist, tau, dtype)
        rounds += 1
        if not r['ok']:
            status = 0
            break
        still = np.abs(r['R32'].astype(np.float64) - R.astype(np.float64)).max() <= np.float64(np.float32(tol_rot)) and \
            np.abs(r['t32'].astype(np.float64) - t.astype(np.float64)).max() <= np.float64(np.float32(tol_trans))
        R, t = r['R32'], r['t32']
        hist.append((R, t))
        if still:
            break
    return dict(R32=R, t32=t, status=status, rounds=rounds, history=hist)


TRUE_R = rotation((0.1, 1.0, 0.05), 0.01)
TRUE_T = np.array([0.03, -0.01, -0.25])


def scene(n, seed, m=None, movers=0.1, clutter=0.1, sigma=0.01):
    """The lidar-like pair of the tests: src uniform in [-15, 15] x [-2, 2] x [2, 35] m; dst = the src moved by 0.01 rad about
    (0.1, 1, 0.05) and t = (0.03, -0.01, -0.25), plus N(0, sigma) noise, floor(movers * n) points displaced by (1, 0, 0.5); its
    columns permuted and floor(clutter * n) of them replaced by uniform clutter.  m: keep the first m columns of dst (or add
    clutter up to m).  -> src (3, n), dst (3, m) float32."""
    rng = np.random.RandomState(seed)
    lo, hi = np.array([-15.0, -2.0, 2.0]), np.array([15.0, 2.0, 35.0])
    p = rng.uniform(lo[:, None], hi[:, None], (3, n))
    q = TRUE_R @ p + TRUE_T[:, None] + rng.normal(0, sigma, (3, n))
    q[:, rng.permutation(n)[:int(movers * n)]] += np.array([[1.0], [0.0], [0.5]])
    q = q[:, rng.permutation(n)]
    k = int(clutter * n)
    q[:, rng.permutation(n)[:k]] = rng.uniform(lo[:, None], hi[:, None], (3, k))
    if m is not None and m != n:
        q = q[:, :m] if m < n else np.concatenate([q, rng.uniform(lo[:, None], hi[:, None], (3, m - n))], 1)
    return p.astype(np.float32), q.astype(np.float32)


def weights(n, seed):
    """Random base weights in [0.5, 1.5) with a tenth of the points switched off (0, negative, NaN or +inf)."""
    rng = np.random.RandomState(2000 + seed)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    off = rng.permutation(n)[:n // 10]
    w[off] = np.array([0.0, -1.0, np.nan, np.inf], np.float32)[np.arange(len(off)) % 4]
    return w
