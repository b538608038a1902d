"""numpy restatement of hpl_motion_segment (include/hpl_bcl.h): the all-pairs float32 predicate in row chunks,
connected components by min-label propagation to a fixed point, the numbering, labels, tables and stats of the definition.
No grid, no dependence on the project or on scipy.  Also the synthetic scene the tests share."""
import numpy as np

F32 = np.float32
CELL_MAX = 2 ** 18 - 2


def movers(pc, flow, residual, tau, eps):
    """-> (mover mask, out-of-range mask) of one pair; pc / flow (3, N) float32, residual (N,) float32."""
    pc, flow, residual = np.asarray(pc, F32), np.asarray(flow, F32), np.asarray(residual, F32)
    with np.errstate(invalid='ignore', over='ignore'):
        cand = (residual > F32(tau)) & np.isfinite(pc).all(0) & np.isfinite(flow).all(0)
        inv = 1.0 / (1.001 * float(F32(eps)))
        cell = np.floor(np.where(np.isfinite(pc), pc, 0).astype(np.float64) * inv)
        inside = (np.abs(cell) <= CELL_MAX).all(0)
    return cand & inside, cand & ~inside


def _dist2(a, b):
    """(da_x^2 + da_y^2) + da_z^2 in float32, every operation rounded: a (3, m), b (3, n) -> (m, n)."""
    with np.errstate(over='ignore', invalid='ignore'):
        d = a[:, :, None] - b[:, None, :]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def edges(P, G, eps, dv, chunk=512):
    """Every ordered pair (i, j) the predicate links (i == j included), from the all-pairs matrix in row chunks."""
    eps2, dv2 = F32(eps) * F32(eps), F32(dv) * F32(dv)
    ii, jj = [], []
    for r in range(0, P.shape[1], chunk):
        i, j = np.nonzero((_dist2(P[:, r:r + chunk], P) <= eps2) & (_dist2(G[:, r:r + chunk], G) <= dv2))
        ii.append(i + r)
        jj.append(j)
    return np.concatenate(ii), np.concatenate(jj)


def components(m, i, j):
    """The smallest index of every node's connected component, by min-label propagation to a fixed point."""
    lab = np.arange(m)
    while True:
        new = lab.copy()
        np.minimum.at(new, i, lab[j])
        new = new[new]
        if np.array_equal(new, lab):
            return lab
        lab = new


def segment(pc, flow, residual, tau=0.1, eps=0.5, dv=float('inf'), min_points=5, max_objects=256):
    """One pair -> dict(labels (N,) int32, obj_info (max_objects, 2) int32, obj_motion (max_objects, 6) float32, stats (4,) int32,
    means (objects, 6) float64: every object's exact float64 mean, also past max_objects)."""
    pc, flow = np.asarray(pc, F32), np.asarray(flow, F32)
    n = pc.shape[1]
    mov, oob = movers(pc, flow, residual, tau, eps)
    idx = np.nonzero(mov)[0]
    root = idx[components(len(idx), *edges(pc[:, idx], flow[:, idx], eps, dv))] if len(idx) else idx
    labels = np.full(n, -1, np.int32)
    labels[oob] = -3
    labels[idx] = -2
    roots, counts = np.unique(root, return_counts=True)            # ascending root order
    keep = counts >= min_points
    roots, counts = roots[keep], counts[keep]
    info = np.tile(np.array([-1, 0], np.int32), (max_objects, 1))
    motion = np.zeros((max_objects, 6), F32)
    means = np.zeros((len(roots), 6), np.float64)
    for o, (r, c) in enumerate(zip(roots, counts)):
        member = idx[root == r]
        labels[member] = o
        means[o] = np.concatenate([pc[:, member].astype(np.float64).mean(1), flow[:, member].astype(np.float64).mean(1)])
        if o < max_objects:
            info[o] = (r, c)
            motion[o] = means[o].astype(F32)
    stats = np.array([len(idx), len(roots), int(counts.sum()), int(oob.sum())], np.int32)
    return dict(labels=labels, obj_info=info, obj_motion=motion, stats=stats, means=means)


def segment_batch(pc, flow, residual, prefix, **kw):
    """A packed batch: every pair on its own.  -> (labels (N,), obj_info (B, M, 2), obj_motion (B, M, 6), stats (B, 4))."""
    outs = [segment(pc[:, a:b], flow[:, a:b], residual[a:b], **kw) for a, b in zip(prefix[:-1], prefix[1:])]
    return (np.concatenate([o['labels'] for o in outs]) if outs else np.zeros(0, np.int32), np.stack([o['obj_info'] for o in outs]),
            np.stack([o['obj_motion'] for o in outs]), np.stack([o['stats'] for o in outs]))


# ----------------------------------------------------------------------------- the scene
def rotation(axis, angle):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


TRUE_R = rotation((0.1, 1, 0.05), 0.03)
TRUE_T = np.array([0.05, -0.02, -0.9])
BOXES = 6
SCENE_KW = dict(tau=0.1, eps=1.0, dv=0.3)


def scene(n, seed=1):
    """A static background under the ego-motion (TRUE_R, TRUE_T) and six boxes of per = max(12, n // 20) points with a flow of
    their own, 1 cm flow noise.  -> (pc (3, n) float32, flow (3, n) float32, residual (n,) float32 against the true motion,
    per); the box points are the last 6 * per, box k the k-th run of per."""
    r = np.random.RandomState(seed)
    per = max(12, n // 20)
    nb = n - BOXES * per
    parts = [np.stack([r.uniform(-15, 15, nb), r.uniform(-2, 2, nb), r.uniform(2, 35, nb)], 1)]
    extra = [np.zeros((nb, 3))]
    for k in range(BOXES):
        c = np.array([-12 + 5 * k, 0.0, 8 + 4 * k])
        parts.append(c + np.stack([r.uniform(-2, 2, per), r.uniform(-0.8, 0.8, per), r.uniform(-0.9, 0.9, per)], 1))
        extra.append(np.tile(np.array([1.0 + 0.3 * k, 0, 0.5 * (-1) ** k]), (per, 1)))
    p = np.concatenate(parts)
    f = (p @ TRUE_R.T + TRUE_T - p) + np.concatenate(extra) + r.normal(0, 0.01, p.shape)
    p32, f32 = np.ascontiguousarray(p.T.astype(F32)), np.ascontiguousarray(f.T.astype(F32))
    P, Fl = p32.astype(np.float64), f32.astype(np.float64)
    res = np.linalg.norm(TRUE_R @ P + TRUE_T[:, None] - (P + Fl), axis=0).astype(F32)
    return p32, f32, res, per
