"""numpy restatement of hpl_icp_plane (include/hpl_bcl.h) for one pair, over icp_oracle.match: the
point-to-plane round, the chained driver and (icp_oracle.finish, unchanged) the finish.  The solve comes by a different method
from the kernel's: np.linalg.eigh where the kernel runs cyclic Jacobi sweeps, and a vectorised sum where the kernel folds
workgroup partials.  `dtype` is the precision of the residuals, the weights and the 28 sums: float64 is the reference, float32
shows what a float32 round over the same matches would lose (the bars of tests/test_gpu_icp_plane.py come from the
difference)."""
import numpy as np

import icp_oracle as P
from normals_oracle import scene as surface

RANK = 1e-10


def valid_normals(nrm):
    nrm = np.asarray(nrm, np.float32)
    with np.errstate(invalid='ignore'):
        return np.isfinite(nrm).all(0) & (nrm != 0).any(0)


def round_(src, dst, nrm, R, t, w=None, max_dist=1.0, tau=0.3, dtype=np.float64, matched=None):
    """One point-to-plane round from the float32 motion (R, t) -> dict(ok, R, t (float64), R32, t32 (what the round hands on;
    the motion it started from when it failed), match, dist2, x (the 6-vector step), lam (eigenvalues of H))."""
    src, dst, nrm = np.asarray(src, np.float32), np.asarray(dst, np.float32), np.asarray(nrm, np.float32)
    R0, t0 = np.asarray(R, np.float32), np.asarray(t, np.float32)
    n, m = src.shape[1], dst.shape[1]
    idx, d2 = P.match(src, dst, R0, t0, max_dist) if matched is None else matched
    fail = dict(ok=False, R=R0.astype(np.float64), t=t0.astype(np.float64), R32=R0, t32=t0, match=idx, dist2=d2)
    if n < 3 or m == 0:
        return fail
    w0 = P.base_weights(src, w)
    j = np.where(idx >= 0, idx, 0)
    live = (w0 > 0) & (idx >= 0) & valid_normals(nrm)[j]
    if not live.any():
        return fail
    with np.errstate(invalid='ignore', over='ignore'):
        y = P.moved(src, R0, t0)[:, live].astype(dtype)
    q = dst[:, j[live]].astype(dtype)
    nn = nrm[:, j[live]].astype(dtype)
    c = np.where(np.isfinite(src[:, 0]), src[:, 0], 0).astype(dtype)
    r = ((y - q) * nn).sum(0, dtype=dtype)
    tau = dtype(np.float32(tau))
    u = (w0[live].astype(dtype) / (1 + r * r / (tau * tau)) ** 2).astype(dtype)
    J = np.concatenate([np.cross((y - c[:, None]).T, nn.T).T, nn]).astype(dtype)          # (6, live)
    W = u.sum(dtype=dtype)
    H = ((J * u) @ J.T).astype(np.float64)
    g = ((J * u) @ r).astype(np.float64)
    if not (W > 0 and np.isfinite(W) and np.isfinite(H).all() and np.isfinite(g).all()):
        return fail
    lam, V = np.linalg.eigh(H)
    if not lam[-1] > 0:
        return fail
    x = np.zeros(6)
    for i in range(6):
        if lam[i] > RANK * lam[-1]:
            x -= V[:, i] * (V[:, i] @ g) / lam[i]
    om, de = x[:3], x[3:]
    th = np.linalg.norm(om)
    K = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    E = np.eye(3) + K if th < 1e-12 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    c64 = c.astype(np.float64)
    Rn = E @ R0.astype(np.float64)
    tn = E @ (t0.astype(np.float64) - c64) + c64 + de
    if not (np.isfinite(Rn).all() and np.isfinite(tn).all()):
        return fail
    return dict(ok=True, R=Rn, t=tn, R32=Rn.astype(np.float32), t32=tn.astype(np.float32), match=idx, dist2=d2, x=x, lam=lam)


def chain(src, dst, nrm, init=None, iters=30, w=None, max_dist=1.0, tau=0.3, tol_rot=0.0, tol_trans=0.0, dtype=np.float64):
    """icp_oracle.chain with the point-to-plane round."""
    src = np.asarray(src, np.float32)
    R, t = (np.asarray(x, np.float32) for x in (P.IDENTITY if init is None else init))
    status = int(src.shape[1] >= 3 and np.asarray(dst).shape[1] > 0)
    rounds, hist = 0, []
    while status and rounds < iters:
        r = round_(src, dst, nrm, R, t, w, max_dist, tau, dtype)
        rounds += 1
        if not r['ok']:
            status = 0
            break
        still = np.abs(r['R32'].astype(np.float64) - R.astype(np.float64)).max() <= np.float64(np.float32(tol_rot)) and \
            np.abs(r['t32'].astype(np.float64) - t.astype(np.float64)).max() <= np.float64(np.float32(tol_trans))
        R, t = r['R32'], r['t32']
        hist.append((R, t, r['match']))
        if still:
            break
    return dict(R32=R, t32=t, status=status, rounds=rounds, history=hist)


finish = P.finish


def pair(n, seed):
    """src and dst drawn INDEPENDENTLY from the same surfaces (normals_oracle.scene with two seeds); dst moved by
    icp_oracle.TRUE_R / TRUE_T.  -> src (3, n), dst (3, n) float32."""
    src = surface(n, 500 + seed)
    dst = P.TRUE_R @ surface(n, 900 + seed).astype(np.float64) + P.TRUE_T[:, None]
    return src, dst.astype(np.float32)
