"""numpy restatement of hpl_object_fit (include/hpl_bcl.h): the members of every object gathered by label in
ascending index, then tests/rigid_oracle.py's fit (an SVD where the kernel takes Horn's quaternion) per object, and the
in-place update of residual and refined.  Also the scene of tests/test_object_fit_cpu.py and tests/test_gpu_object_fit.py."""
import numpy as np

import rigid_oracle

#: member counts of the scene's objects: a lane's last slot (255, 256, 257), a span's edge in both directions (1023, 1024,
#: 1025), two and three spans (1025, 2049), and the 17th span that wraps fold_partials' 16 strided runs (17 409 = 17 * 1024 + 1)
SIZES = (1, 2, 3, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 17409)
MAX_OBJECTS = 16
OTHERS = 692                     # points of no object: labels -1, -2, -3 and max_objects + 7 in turn
N = sum(SIZES) + OTHERS          # 24 001
SEED = 6                         # (chosen so that no residual lies within 1e-4 of tau: tests/test_object_fit_cpu.py checks it)
TAU = 0.1


def members(labels, prefix, b, o):
    """The packed indices of object o of pair b, ascending."""
    return prefix[b] + np.flatnonzero(np.asarray(labels[prefix[b]:prefix[b + 1]]) == o)


def fit_objects(p, f, labels, w=None, max_objects=MAX_OBJECTS, iters=4, tau=TAU, prefix=None, residual=None, refined=None,
                dtype=np.float64):
    """p, f (3, N) float32, labels (N) -> (fits, residual, refined): fits[b][o] = rigid_oracle.fit's dict of object o of pair b
    with its `members`, or None for an object without members; residual (N) float64 and refined (N, 3) float32 are copies of
    the arrays handed in (None: NaN), updated as the op updates them."""
    n = p.shape[1]
    prefix = [0, n] if prefix is None else list(prefix)
    residual = np.full(n, np.nan) if residual is None else np.array(residual, np.float64)
    refined = np.full((n, 3), np.nan, np.float32) if refined is None else np.array(refined, np.float32)
    fits = []
    for b in range(len(prefix) - 1):
        row = []
        for o in range(max_objects):
            idx = members(labels, prefix, b, o)
            if not len(idx):
                row.append(None)
                continue
            fit = rigid_oracle.fit(p[:, idx], f[:, idx], None if w is None else w[idx], iters, tau, dtype)
            fit['members'] = idx
            residual[idx] = fit['residual']
            refined[idx[fit['inlier']]] = fit['refined'][fit['inlier']]
            row.append(fit)
        fits.append(row)
    return fits, residual, refined


def motions(seed=SEED):
    """The objects' true motions: (R (3, 3), t (3,)) each, rotations of up to 0.2 rad and translations of up to 1.5 m."""
    rng = np.random.RandomState(100 + seed)
    return [(rigid_oracle.rotation(rng.normal(size=3), rng.uniform(0.02, 0.2)), rng.uniform(-1.5, 1.5, 3)) for _ in SIZES]


def scene(seed=SEED, max_objects=MAX_OBJECTS, sigma=0.01):
    """One pair of N = 24 001 points: object k of SIZES[k] members in a 4 m box of its own with its own rigid motion, float32
    flow noise sigma, and a fifth of its members displaced by a further 1 to 2 m -- well beyond tau --; OTHERS background points
    labelled -1, -2, -3 and max_objects + 7 in turn.  All of it interleaved by one fixed permutation, so that no object is a
    contiguous range and the gather is never the identity.  -> (p, f (3, N) float32, labels (N) int32, outlier (N) bool)."""
    rng = np.random.RandomState(seed)
    ps, fs, ls, outs = [], [], [], []
    for k, ((R, t), n) in enumerate(zip(motions(seed), SIZES)):
        c = np.array([-14.0 + 2.5 * k, 0.0, 6.0 + 2.0 * k])
        p = c[:, None] + rng.uniform(-2, 2, (3, n))
        f = R @ p + t[:, None] - p + rng.normal(0, sigma, (3, n))
        out = np.zeros(n, bool)
        out[rng.permutation(n)[:n // 5]] = True
        push = rng.normal(size=(3, n))
        f[:, out] += (push / np.linalg.norm(push, axis=0) * rng.uniform(1.0, 2.0, n))[:, out]
        ps.append(p), fs.append(f), ls.append(np.full(n, k)), outs.append(out)
    ps.append(np.stack([rng.uniform(-15, 15, OTHERS), rng.uniform(-2, 2, OTHERS), rng.uniform(2, 35, OTHERS)]))
    fs.append(rng.normal(0, 0.3, (3, OTHERS)))
    ls.append(np.array([-1, -2, -3, max_objects + 7])[np.arange(OTHERS) % 4])
    outs.append(np.zeros(OTHERS, bool))
    order = rng.permutation(N)
    return (np.concatenate(ps, 1)[:, order].astype(np.float32), np.concatenate(fs, 1)[:, order].astype(np.float32),
            np.concatenate(ls)[order].astype(np.int32), np.concatenate(outs)[order])


def with_non_finite(p, f, labels, w):
    """A variant of the scene with, on labelled points of the large objects, a NaN coordinate, an infinite flow component and
    weights of 0, NaN and inf; and with the whole of object 6 switched off (W = 0: status 0).  -> copies (p, f, w)."""
    p, f, w = p.copy(), f.copy(), w.copy()
    big = np.flatnonzero(labels == 11)
    p[0, big[3]], p[2, big[700]] = np.nan, np.inf
    f[1, big[5]], f[0, big[1030]] = np.inf, -np.inf
    w[big[7]], w[big[8]], w[big[9]], w[big[2000]] = 0.0, np.nan, np.inf, -1.0
    first = np.flatnonzero(labels == 10)[0]                    # an object's pivot that is not finite counts as 0
    p[1, first] = np.nan
    w[labels == 6] = 0.0
    return p, f, w
