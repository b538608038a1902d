"""numpy restatement of hpl_ground_fit (include/hpl_bcl.h): every rule in float64 from the float32 inputs, one
rounded operation at a time in the header's order, so the integer votes, the winner and the classification are the library's
exactly; the refinement takes its eigenvector from numpy.linalg.eigh instead of Jacobi sweeps, and its sums in numpy's order.
Philox4x32-10 is restated too (pinned against the library's host entry in tests/test_ground_cpu.py).  Also the scene
generator of the ground tests: a tilted noisy ground sheet, uniform clutter above it and a vertical wall."""
import math

import numpy as np

PURPOSE = 16                 # the counter's fourth word of the hypotheses' draws
U64 = np.uint64
MASK = U64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter (..., 4) and key (2,) of uint32 values -> (..., 4) uint32."""
    counter = np.asarray(counter)
    c = [counter[..., i].astype(U64) for i in range(4)]
    k0, k1 = U64(int(key[0])), U64(int(key[1]))
    for r in range(10):
        if r:
            k0, k1 = (k0 + U64(0x9E3779B9)) & MASK, (k1 + U64(0xBB67AE85)) & MASK
        p0, p1 = U64(0xD2511F53) * c[0], U64(0xCD9E8D57) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> U64(32)) ^ c[3] ^ k1, p0 & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def draws(n, hyps, seed, call):
    """The three point indices (within a cloud of n points) of hypotheses 0 .. hyps - 1: (hyps, 3) int64."""
    cnt = np.empty((hyps, 4), np.uint32)
    cnt[:, 0] = np.arange(hyps)
    cnt[:, 1], cnt[:, 2], cnt[:, 3] = call & 0xFFFFFFFF, (call >> 32) & 0xFFFFFFFF, PURPOSE
    r = philox4x32_10(cnt, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return ((r[:, :3].astype(U64) * U64(n)) >> U64(32)).astype(np.int64)


def min_cos_of(max_tilt_deg):
    """The float32 cosine ops.ground_fit hands to the library."""
    return np.float32(math.cos(math.radians(float(max_tilt_deg))))


def _f64(v):
    return np.float64(np.float32(v))


def _gate(up, min_cos):
    up = np.asarray(up, np.float32).astype(np.float64)
    mc = _f64(min_cos)
    return up, (mc * mc) * ((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2])


def hypotheses(pc, up, min_cos, hyps, tau, seed, call):
    """-> (a (3, H), m (3, H), q (H,), valid (H,)) of one cloud pc (3, n) float32."""
    n = pc.shape[1]
    if n < 3:
        return np.zeros((3, hyps)), np.zeros((3, hyps)), np.full(hyps, -1.0), np.zeros(hyps, bool)
    P = pc.astype(np.float64)
    fin = np.isfinite(pc).all(0)
    up, gate = _gate(up, min_cos)
    i = draws(n, hyps, seed, call)
    with np.errstate(all='ignore'):
        a = P[:, i[:, 0]]
        u, v = P[:, i[:, 1]] - a, P[:, i[:, 2]] - a
        m = np.stack([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
        q = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
        c = (m[0] * up[0] + m[1] * up[1]) + m[2] * up[2]
        neg = c < 0
        m[:, neg] = -m[:, neg]
        c[neg] = -c[neg]
        valid = fin[i[:, 0]] & fin[i[:, 1]] & fin[i[:, 2]] & (q > 0) & np.isfinite(q) & (c * c >= gate * q)
    return a, m, q, valid


def count_votes(pc, a, m, q, valid, tau, chunk=32):
    """votes (H,) int32: the valid points with s s <= (tau tau) q; -1 for an invalid hypothesis."""
    P = pc.astype(np.float64)
    fin = np.isfinite(pc).all(0)
    t = _f64(tau)
    thr = (t * t) * q
    out = np.full(len(q), -1, np.int32)
    with np.errstate(all='ignore'):
        for h0 in range(0, len(q), chunk):
            sl = slice(h0, h0 + chunk)
            A, M = a[:, sl, None], m[:, sl, None]
            s = (M[0] * (P[0][None] - A[0]) + M[1] * (P[1][None] - A[1])) + M[2] * (P[2][None] - A[2])
            cnt = (fin[None] & (s * s <= thr[sl, None])).sum(1)
            out[sl] = np.where(valid[sl], cnt, -1)
    return out


def heights(pc, plane):
    """h_i = ((n_x x + n_y y) + n_z z) + d in float64 for plane (4,) of any float type."""
    P, pl = pc.astype(np.float64), np.asarray(plane).astype(np.float64)
    with np.errstate(all='ignore'):
        return ((pl[0] * P[0] + pl[1] * P[1]) + pl[2] * P[2]) + pl[3]


def fit(pc, up=(0, 1, 0), min_cos=None, hyps=256, tau=0.1, refine=2, seed=0, call=0, max_tilt_deg=20.0):
    """One cloud.  -> dict(status, h, votes (its count), all_votes (H,), plane64 (4,), plane (4,) float32, rounds: the
    refinement rounds that took effect)."""
    min_cos = min_cos_of(max_tilt_deg) if min_cos is None else min_cos
    a, m, q, valid = hypotheses(pc, up, min_cos, hyps, tau, seed, call)
    votes = count_votes(pc, a, m, q, valid, tau)
    best = int(np.argmax(votes))                  # the first of the largest: the smallest h among equals
    if votes[best] < 0:
        return dict(status=0, h=-1, votes=0, all_votes=votes, plane64=np.zeros(4), plane=np.zeros(4, np.float32), rounds=0)
    nn = m[:, best] / np.sqrt(q[best])
    piv = a[:, best]
    d = -((nn[0] * piv[0] + nn[1] * piv[1]) + nn[2] * piv[2])
    upv, gate = _gate(up, min_cos)
    P, fin, t = pc.astype(np.float64), np.isfinite(pc).all(0), _f64(tau)
    rounds = 0
    for _ in range(refine):
        with np.errstate(all='ignore'):
            inl = fin & (np.abs(heights(pc, np.append(nn, d))) <= t)
        W = float(inl.sum())
        if W < 3:
            break
        dp = P[:, inl] - piv[:, None]
        mu = dp.sum(1) / W
        C = dp @ dp.T - np.outer(W * mu, mu)
        if not np.isfinite(C).all():
            break
        v = np.linalg.eigh(C)[1][:, 0]
        v = v / np.sqrt(v @ v)
        c = v @ upv
        if c < 0:
            v, c = -v, -c
        dd = -(v @ (piv + mu))
        if not (np.isfinite(v).all() and np.isfinite(dd) and c * c >= gate * (v @ v)):
            break
        nn, d, rounds = v, dd, rounds + 1
    p64 = np.append(nn, d)
    return dict(status=1, h=best, votes=int(votes[best]), all_votes=votes, plane64=p64, plane=p64.astype(np.float32), rounds=rounds)


def classify(pc, plane, status, cut):
    """One cloud against the float32 plane (4,): -> (height (n,) float32, ground (n,) uint8, keep (n,) bool)."""
    n = pc.shape[1]
    if not status:
        return np.zeros(n, np.float32), np.zeros(n, np.uint8), np.ones(n, bool)
    fin = np.isfinite(pc).all(0)
    h = heights(pc, np.asarray(plane, np.float32))
    with np.errstate(all='ignore'):
        gr = fin & (h <= _f64(cut))
        return np.where(fin, h.astype(np.float32), np.float32(np.nan)), gr.astype(np.uint8), ~gr


def classify_batch(pc, prefix, plane, status, cut):
    """The packed classification outputs for given float32 planes (B, 4) and statuses (B,):
    -> (height (N,), ground (N,), keep_idx (N,) int32, kept (B,))."""
    N = pc.shape[1]
    height, ground = np.zeros(N, np.float32), np.zeros(N, np.uint8)
    keep_idx, kept = np.full(N, -1, np.int32), []
    for b in range(len(prefix) - 1):
        p0, p1 = prefix[b], prefix[b + 1]
        hb, gb, kb = classify(pc[:, p0:p1], plane[b], status[b], cut)
        height[p0:p1], ground[p0:p1] = hb, gb
        idx = np.flatnonzero(kb) + p0
        keep_idx[p0:p0 + len(idx)] = idx
        kept.append(len(idx))
    return height, ground, keep_idx, np.asarray(kept, np.int32)


def ground_fit(pc, prefix=None, up=(0, 1, 0), max_tilt_deg=20.0, hyps=256, tau=0.1, refine=2, cut=0.3, seed=0, call=0):
    """ops.ground_fit's outputs for a packed batch: dict(plane (B, 4) float32, plane64, stats (B, 4) int32, ground, keep_idx,
    votes (B, H), height)."""
    prefix = [0, pc.shape[1]] if prefix is None else list(prefix)
    fits = [fit(pc[:, prefix[b]:prefix[b + 1]], up, None, hyps, tau, refine, seed, call, max_tilt_deg) for b in range(len(prefix) - 1)]
    plane = np.stack([f['plane'] for f in fits])
    status = [f['status'] for f in fits]
    height, ground, keep_idx, kept = classify_batch(pc, prefix, plane, status, cut)
    stats = np.array([[f['status'], f['h'], f['votes'], k] for f, k in zip(fits, kept)], np.int32).reshape(-1, 4)
    return dict(plane=plane, plane64=np.stack([f['plane64'] for f in fits]), stats=stats, ground=ground, keep_idx=keep_idx,
                votes=np.stack([f['all_votes'] for f in fits]), height=height, rounds=[f['rounds'] for f in fits])


# ----------------------------------------------------------------------------- scenes
AXES = {'x': 0, 'y': 1, 'z': 2}


def scene(n, seed, ground=0.5, wall=0.0, tilt_deg=5.0, height=1.6, noise=0.03, up='y', extent=20.0):
    """A cloud (3, n) float32 in random order: a ground sheet of round(ground n) points whose normal tilts tilt_deg from the up
    axis, `height` below the origin, with normal noise of sigma `noise` along it; a vertical wall of round(wall n) points (a
    plane through the up axis, 8 m out, 6 m tall, the same noise); uniform clutter 0.5 .. 3 m above the sheet for the rest.
    -> (pc, truth): truth = dict(normal (3,), d, wall_normal (3,), up (3,)) with the ground n . x + d = 0, n . up > 0."""
    rng = np.random.RandomState(seed)
    k = AXES[up]
    e_up, h1, h2 = np.eye(3)[k], np.eye(3)[(k + 1) % 3], np.eye(3)[(k + 2) % 3]
    t = math.radians(tilt_deg)
    nrm = math.cos(t) * e_up + math.sin(t) * h1                # tilted about h2
    t1, t2 = math.cos(t) * h1 - math.sin(t) * e_up, h2
    c0 = -height * e_up
    ng, nw = int(round(ground * n)), int(round(wall * n))
    nc = n - ng - nw

    def sheet(cnt, lo, hi, sigma):
        s1, s2 = rng.uniform(-extent, extent, cnt), rng.uniform(-extent, extent, cnt)
        hgt = rng.uniform(lo, hi, cnt) + rng.normal(0, 1, cnt) * sigma
        return c0[:, None] + t1[:, None] * s1 + t2[:, None] * s2 + nrm[:, None] * hgt

    parts = [sheet(ng, 0.0, 0.0, noise), sheet(nc, 0.5, 3.0, 0.0)]
    w = c0[:, None] + h1[:, None] * (8.0 + rng.normal(0, 1, nw) * noise) + h2[:, None] * rng.uniform(-extent, extent, nw) + \
        e_up[:, None] * rng.uniform(0.0, 6.0, nw)
    pc = np.concatenate(parts + [w], axis=1)[:, rng.permutation(n)].astype(np.float32)
    return pc, dict(normal=nrm, d=float(-(nrm @ c0)), wall_normal=h1, up=e_up)


def angle_deg(u, v):
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    c = abs(u @ v) / math.sqrt((u @ u) * (v @ v))
    s = np.linalg.norm(np.cross(u, v)) / math.sqrt((u @ u) * (v @ v))
    return math.degrees(math.atan2(s, c))
