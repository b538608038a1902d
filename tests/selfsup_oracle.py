"""numpy restatement of hpl_selfsup_loss (include/hpl_bcl.h): all pairs, no tiling.  The searches in float32
with the library's own operations, order and tie rule (tests/knn_oracle.py is the model), so the neighbour assignments are the
kernel's exactly; the sums and the gradient in float64, the incoming sums in ascending source order (np.add.at adds in the
order of its index array).

real=np.float64 evaluates the same definition with the warped points and the search in float64: the function of real
numbers whose gradient the finite-difference test of tests/test_selfsup_cpu.py checks."""
import numpy as np

INF_BITS = np.uint64(0x7f800000)


def nearest(ref, q, k, exclude_self=False, real=np.float32):
    """ref (3, N), q (3, n) of one pair -> idx (k, n) int32 (-1: absent), d2 (k, n): ascending, ties to the smaller index, a d2
    that is not below +inf (NaN included) never enters.  exclude_self: query i leaves reference i out (by index)."""
    N, n = ref.shape[1], q.shape[1]
    idx = np.full((k, n), -1, np.int32)
    out = np.full((k, n), np.inf, real)
    if N == 0 or n == 0 or k == 0:
        return idx, out
    with np.errstate(invalid='ignore', over='ignore'):
        dx = q[0][:, None] - ref[0][None, :]             # arrays of `real`: every operation rounds to it
        dy = q[1][:, None] - ref[1][None, :]
        dz = q[2][:, None] - ref[2][None, :]
        d2 = (dx * dx + dy * dy) + dz * dz
    d2 = np.where(d2 < np.inf, d2, np.inf).astype(real)  # (NaN fails the comparison)
    if exclude_self:
        d2[np.arange(n), np.arange(n)] = np.inf
    order = np.argsort(d2, axis=1, kind='stable')        # stable: equal d2 keep index order
    kk = min(k, N)
    top = order[:, :kk]
    dd = np.take_along_axis(d2, top, axis=1)
    found = dd < np.inf
    idx[:kk] = np.where(found, top, -1).T
    out[:kk] = np.where(found, dd, np.inf).T
    return idx, out


def pair(pc1, flow, pc2, k, wc, ws, real=np.float32):
    """One pair: pc1, flow (3, N1), pc2 (3, N2) float32 -> dict of float64 results and the assignments (pair-local).
    real=np.float64 also takes the inputs as float64 (a flow stepped by a finite difference is not rounded)."""
    x, f, q = (np.asarray(t, real) for t in (pc1, flow, pc2))
    n1, n2 = x.shape[1], q.shape[1]
    wc, ws = np.float64(np.float32(wc)), np.float64(np.float32(ws))
    with np.errstate(invalid='ignore', over='ignore'):
        p = (x.astype(real) + f.astype(real)).astype(real)               # rounded once
    qq = q.astype(real)
    a, d12 = nearest(qq, p, 1, real=real)
    b, d21 = nearest(p, qq, 1, real=real)
    a, b, d12, d21 = a[0], b[0], d12[0].astype(np.float64), d21[0].astype(np.float64)
    nbr, _ = nearest(x, x, k, exclude_self=True, real=real)
    ki = (nbr >= 0).sum(0)                                               # (n1,)
    P, Q, F = p.astype(np.float64).T, q.astype(np.float64).T, f.astype(np.float64).T      # point-major
    C12 = C21 = S = 0.0
    if n1 > 0 and n2 > 0:
        C12 = np.where(a >= 0, d12, 0.0).sum() / n1
        C21 = np.where(b >= 0, d21, 0.0).sum() / n2
    B = np.zeros((n1, 3))
    C = np.zeros((n1, 3))
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        if n1 > 0 and k > 0:
            s = np.zeros(n1)
            for r in range(k):
                ok = nbr[r] >= 0
                d = F - F[np.where(ok, nbr[r], 0)]
                s = s + np.where(ok, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], 0.0)
                B = B + np.where(ok[:, None], d, 0.0)
            S = np.where(ki > 0, s / np.maximum(ki, 1), 0.0).sum() / n1
            tgt = nbr.T.reshape(-1)                                      # source-major: ascending m for every target
            src = np.repeat(np.arange(n1), k)
            ok = tgt >= 0
            tgt, src = tgt[ok], src[ok]
            np.add.at(C, tgt, (F[tgt] - F[src]) * (1.0 / ki[src])[:, None])
        L = wc * (C12 + C21)
        if k > 0:
            L = L + ws * S
        own = np.where((a >= 0)[:, None], P - Q[np.where(a >= 0, a, 0)], 0.0) if n2 > 0 else np.zeros((n1, 3))
        A = np.zeros((n1, 3))
        js = np.nonzero(b >= 0)[0]                                       # ascending j
        np.add.at(A, b[js], P[b[js]] - Q[js])
        g = np.zeros((n1, 3))
        if n1 > 0:
            s1, s2 = 2.0 / n1, (2.0 / n2 if n2 > 0 else 0.0)
            g = wc * (s1 * own + s2 * A)
            if k > 0:
                g = g + ws * (s1 * (np.where((ki > 0)[:, None], B / np.maximum(ki, 1)[:, None], 0.0) + C))
    return {'L': L, 'C12': C12, 'C21': C21, 'S': S, 'dflow': g, 'nn12': a, 'nn21': b, 'nbr': nbr}


def selfsup(pc1, flow, pc2, k=8, wc=1.0, ws=1.0, prefix1=None, prefix2=None, real=np.float32):
    """Packed pairs: pc1, flow (3, N1), pc2 (3, N2) -> dict(loss (B, 4) float32 and loss64, dflow (N1, 3) float32 and dflow64,
    nn12 (N1), nn21 (N2), nbr (k, N1) int32 into the packed arrays, -1 where absent)."""
    pc1, flow, pc2 = (np.asarray(t, np.float32) for t in (pc1, flow, pc2))
    N1, N2 = pc1.shape[1], pc2.shape[1]
    p1 = [0, N1] if prefix1 is None else list(prefix1)
    p2 = [0, N2] if prefix2 is None else list(prefix2)
    B = len(p1) - 1
    loss = np.zeros((B, 4))
    g = np.zeros((N1, 3))
    nn12 = np.full(N1, -1, np.int32)
    nn21 = np.full(N2, -1, np.int32)
    nbr = np.full((k, N1), -1, np.int32)
    for b in range(B):
        s1, s2 = slice(p1[b], p1[b + 1]), slice(p2[b], p2[b + 1])
        o = pair(pc1[:, s1], flow[:, s1], pc2[:, s2], k, wc, ws, real)
        loss[b] = (o['L'], o['C12'], o['C21'], o['S'])
        g[s1] = o['dflow']
        nn12[s1] = np.where(o['nn12'] >= 0, o['nn12'] + p2[b], -1)
        nn21[s2] = np.where(o['nn21'] >= 0, o['nn21'] + p1[b], -1)
        nbr[:, s1] = np.where(o['nbr'] >= 0, o['nbr'] + p1[b], -1)
    with np.errstate(over='ignore', invalid='ignore'):
        return {'loss': loss.astype(np.float32), 'loss64': loss, 'dflow': g.astype(np.float32), 'dflow64': g, 'nn12': nn12,
                'nn21': nn21, 'nbr': nbr}
