"""numpy restatement of hpl_rigid_fit (include/hpl_bcl.h) by a different method: the rotation comes from a
float64 SVD (Kabsch, with the determinant fix), where the kernel takes Horn's quaternion from Jacobi sweeps.  The weights, the
Geman-McClure update, the inlier rule and the status-0 rule are the interface's.  `dtype` is the precision of the centroids,
the covariance and the residuals: float64 is the reference, float32 shows what a float32 fit of the same input would lose."""
import numpy as np


def kabsch(H):
    """The proper rotation R maximising tr(R H), H = sum u (p - mp)(q - mq)^T (3, 3), in float64."""
    U, _, Vt = np.linalg.svd(np.asarray(H, np.float64))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    D = np.diag([1.0, 1.0, d if d != 0 else 1.0])
    return Vt.T @ D @ U.T


def base_weights(p, f, w):
    """The effective base weights (float64): w (or 1), 0 where w is not in (0, inf) or the point or its flow is not finite."""
    n = p.shape[1]
    w = np.ones(n, np.float32) if w is None else np.asarray(w, np.float32)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(p).all(0) & np.isfinite(f).all(0) & (w > 0) & np.isfinite(w)
    return np.where(ok, w, 0).astype(np.float64)


def fit(p, f, w=None, iters=4, tau=0.1, dtype=np.float64):
    """p, f (3, n) float32, w (n) or None -> dict(R (3, 3), t (3,), status, residual (n), inlier (n) bool, refined (n, 3)
    float32, share, angle_deg, trans), the outputs of hpl_rigid_fit for one pair."""
    p32, f32 = np.asarray(p, np.float32), np.asarray(f, np.float32)
    n = p32.shape[1]
    w0 = base_weights(p32, f32, w).astype(dtype)
    live = w0 > 0
    P = np.where(live, p32, 0).astype(dtype)             # (points of weight 0 take no part: keep their NaNs out)
    Q = P + np.where(live, f32, 0).astype(dtype)
    tau = dtype(np.float32(tau))
    R, t, status = np.eye(3), np.zeros(3), n >= 3
    u = w0.copy()
    for k in range(iters + 1):
        W = u.sum(dtype=dtype)
        if not (status and W > 0 and np.isfinite(W)):
            status = False
            break
        mp, mq = (P * u).sum(1, dtype=dtype) / W, (Q * u).sum(1, dtype=dtype) / W
        dp, dq = P - mp[:, None], Q - mq[:, None]
        H = (dp * u) @ dq.T
        R = kabsch(H)
        t = mq.astype(np.float64) - R @ mp.astype(np.float64)
        if k < iters:
            r = np.sqrt((((R.astype(dtype) @ P + t.astype(dtype)[:, None]) - Q) ** 2).sum(0, dtype=dtype))
            u = w0 / (1 + (r / tau) ** 2) ** 2
    if not status:
        R, t = np.eye(3), np.zeros(3)
    with np.errstate(invalid='ignore'):
        pd, fd = p32.astype(dtype), f32.astype(dtype)
        moved = R.astype(dtype) @ pd + t.astype(dtype)[:, None]
        r = np.sqrt(((moved - (pd + fd)) ** 2).sum(0, dtype=dtype))
        inlier = (r <= tau) & live & bool(status)
    refined = f32.T.copy()
    refined[inlier] = (moved - pd).T[inlier].astype(np.float32)
    c = np.clip((np.trace(R) - 1) / 2, -1, 1)
    return dict(R=R, t=t, status=int(bool(status)), residual=r, inlier=inlier, refined=refined,
                share=float(inlier.sum()) / max(n, 1), angle_deg=float(np.degrees(np.arccos(c))) if status else 0.0,
                trans=float(np.linalg.norm(t)))


def rotation(axis, angle):
    """Rodrigues: the rotation by `angle` (rad) about `axis`, float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


TRUE_R = rotation((0.1, 1.0, 0.05), 0.03)
TRUE_T = np.array([0.05, -0.02, -0.9])


def scene(n, seed, movers=0.25, sigma=0.01):
    """The lidar-like scene of the tests: p uniform in [-15, 15] x [-2, 2] x [2, 35] m, one rigid motion (0.03 rad about
    (0.1, 1, 0.05), t = (0.05, -0.02, -0.9)), flow noise sigma, and floor(movers * n) points that carry an extra (1, 0, 0.5).
    -> p, f (3, n) float32, static (n) bool."""
    rng = np.random.RandomState(seed)
    p = np.stack([rng.uniform(-15, 15, n), rng.uniform(-2, 2, n), rng.uniform(2, 35, n)])
    f = TRUE_R @ p + TRUE_T[:, None] - p + rng.normal(0, sigma, (3, n))
    static = np.ones(n, bool)
    static[rng.permutation(n)[:int(movers * n)]] = False
    f[:, ~static] += np.array([[1.0], [0.0], [0.5]])
    return p.astype(np.float32), f.astype(np.float32), static


def weights(n, seed):
    """Random base weights in [0.5, 1.5) with a tenth of the points switched off (0, negative or NaN)."""
    rng = np.random.RandomState(1000 + seed)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    off = rng.permutation(n)[:n // 10]
    w[off] = np.array([0.0, -1.0, np.nan], np.float32)[np.arange(len(off)) % 3]
    return w
