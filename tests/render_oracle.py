"""numpy restatement of hpl_render_maps / hpl_maps_to_kitti (include/hpl_bcl.h) with all points and no atomics:
per pixel the lexicographic minimum of (bits(zc), local index) over the points whose footprint covers the pixel, found by one
sort.  Every float32 operation is one numpy float32 operation in the order the header states.  Also the scene generators of
test_render_cpu.py and test_gpu_render.py.
"""
import numpy as np

f32 = np.float32
KITTI_NEAR = f32(1e-3)


def camera_of_P(P):
    """(f, cx, cy, constx, consty, constz) of a P_rect_02, as data.read_kitti_camera derives it."""
    P = np.asarray(P, dtype=f32).reshape(3, 4)
    return tuple(f32(v) for v in (-P[0, 0], P[0, 2], P[1, 2], P[0, 3], P[1, 3], P[2, 3]))


def project(pc, camera):
    """pc [n, 3] float32 -> (zc, u, v) float32 [n], the order of utils/geometry.py:project_3d_to_2d."""
    f, cx, cy, kx, ky, kz = (f32(c) for c in camera)
    X, Y, Z = (np.ascontiguousarray(pc[:, k], dtype=f32) for k in range(3))
    with np.errstate(all='ignore'):
        zc = Z + kz
        u = ((X * f + cx * Z) + kx) / zc
        v = ((Y * f + cy * Z) + ky) / zc
    return zc, u, v


def projectable(pc, zc, near):
    with np.errstate(all='ignore'):
        return np.isfinite(pc).all(axis=1) & (zc >= f32(near))


def _pixels(pc, camera, H, W, near):
    """(ok, inside, i, j, zc, u, v): the tests on the floats, the indices only where inside."""
    zc, u, v = project(pc, camera)
    ok = projectable(pc, zc, near)
    with np.errstate(all='ignore'):
        ru, rv = np.rint(u), np.rint(v)
        inside = ok & (ru >= 0) & (ru.astype(np.float64) <= W - 1) & (rv >= 0) & (rv.astype(np.float64) <= H - 1)
    j = np.where(inside, ru, 0).astype(np.int64)
    i = np.where(inside, rv, 0).astype(np.int64)
    return ok, inside, i, j, zc, u, v


def zbuffer(inside, i, j, zc, H, W, footprint):
    """-> (winner [H * W] int32 or -1, zbits [H * W] uint32): per pixel the smallest (bits(zc), index) among the inside points
    whose (2 footprint + 1)^2 square covers it."""
    idx = np.flatnonzero(inside)
    bits = zc.view(np.uint32)[idx].astype(np.int64)
    cand_px, cand_bits, cand_idx = [], [], []
    for dy in range(-footprint, footprint + 1):
        for dx in range(-footprint, footprint + 1):
            ii, jj = i[idx] + dy, j[idx] + dx
            keep = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
            cand_px.append((ii * W + jj)[keep])
            cand_bits.append(bits[keep])
            cand_idx.append(idx[keep])
    px, bt, ix = (np.concatenate(c) if c else np.zeros(0, np.int64) for c in (cand_px, cand_bits, cand_idx))
    order = np.lexsort((ix, bt, px))
    px, bt, ix = px[order], bt[order], ix[order]
    first = np.ones(len(px), bool)
    first[1:] = px[1:] != px[:-1]
    winner = np.full(H * W, -1, np.int32)
    zbits = np.zeros(H * W, np.uint32)
    winner[px[first]] = ix[first]
    zbits[px[first]] = bt[first]
    return winner, zbits


def render_maps(pc, camera, H, W, attrs=None, footprint=0, rel_tol=0.0, abs_tol=0.0, near=1e-3):
    """pc [n, 3] float32 of ONE cloud, attrs [C, n] or None -> dict of pixel_of [n] int32, winner [H * W] int32, depth [H * W]
    float32, attr_map [C, H * W] or None, visible [n] uint8, stats [4] int32."""
    pc = np.ascontiguousarray(pc, dtype=f32).reshape(-1, 3)
    n = len(pc)
    ok, inside, i, j, zc, _, _ = _pixels(pc, camera, H, W, near)
    pixel_of = np.where(inside, i * W + j, -1).astype(np.int32)
    winner, zbits = zbuffer(inside, i, j, zc, H, W, footprint)
    covered = winner >= 0
    depth = np.where(covered, zbits.view(f32), f32(0)).astype(f32)
    attr_map = None
    if attrs is not None:
        attrs = np.asarray(attrs, dtype=f32)
        attrs = attrs.reshape(attrs.shape[0] if attrs.ndim == 2 else 1, n)
        attr_map = np.zeros((len(attrs), H * W), f32)
        attr_map[:, covered] = attrs[:, winner[covered]]
    rel1 = f32(1) + f32(rel_tol)
    with np.errstate(all='ignore'):
        zmin = depth[np.where(inside, pixel_of, 0)] if H * W else np.zeros(n, f32)
        visible = inside & (zc <= (zmin * rel1) + f32(abs_tol))
    stats = np.array([inside.sum(), covered.sum(), visible.sum(), n - ok.sum()], np.int32)
    return dict(pixel_of=pixel_of, winner=winner, depth=depth, attr_map=attr_map, visible=visible.astype(np.uint8), stats=stats)


def _raw16(x, lo, hi):
    """rint(x) clamped to lo .. hi as uint16; a NaN gives lo."""
    with np.errstate(all='ignore'):
        r = np.rint(x)
        return np.where(r >= f32(lo), np.where(r <= f32(hi), r, f32(hi)), f32(lo)).astype(np.int64).astype(np.uint16)


def maps_to_kitti(pc1, pc2, P, H, W, baseline=0.54, footprint=0):
    """pc1, pc2 [n, 3] float32 of ONE frame -> (disp1 (H, W) uint16, disp2 (H, W), flow (H, W, 3))."""
    pc1 = np.ascontiguousarray(pc1, dtype=f32).reshape(-1, 3)
    pc2 = np.ascontiguousarray(pc2, dtype=f32).reshape(-1, 3)
    P = np.asarray(P, dtype=f32).reshape(3, 4)
    cam = camera_of_P(P)
    fb = P[0, 0] * f32(baseline)
    _, inside, i, j, zc, _, _ = _pixels(pc1, cam, H, W, KITTI_NEAR)
    winner, _ = zbuffer(inside, i, j, zc, H, W, footprint)
    covered = winner >= 0
    w = np.where(covered, winner, 0)
    d1, d2 = np.zeros(H * W, np.uint16), np.zeros(H * W, np.uint16)
    flow = np.zeros((H * W, 3), np.uint16)
    if len(pc1) and H * W:
        a, b = pc1[w], pc2[w]
        zc2, px2, py2 = project(b, cam)
        ok2 = covered & projectable(b, zc2, KITTI_NEAR)
        col = (np.arange(H * W) % W).astype(f32)
        row = (np.arange(H * W) // W).astype(f32)
        with np.errstate(all='ignore'):
            r1 = _raw16((fb / a[:, 2] - f32(1e-5)) * f32(256), 1, 65535)
            r2 = _raw16((fb / b[:, 2] - f32(1e-5)) * f32(256), 1, 65535)
            u = _raw16((px2 - col) * f32(64) + f32(32768), 0, 65535)
            v = _raw16((py2 - row) * f32(64) + f32(32768), 0, 65535)
        d1 = np.where(covered, r1, 0).astype(np.uint16)
        d2 = np.where(ok2, r2, 0).astype(np.uint16)
        flow[:, 0], flow[:, 1], flow[:, 2] = np.where(ok2, u, 0), np.where(ok2, v, 0), ok2
    return d1.reshape(H, W), d2.reshape(H, W), flow.reshape(H, W, 3)


def valid_kitti(disp1, disp2, flow):
    return (disp1 > 0) & (disp2 > 0) & (flow[..., 2] == 1)


def expected_raw(disp1, disp2, flow):
    """What the round trip must return: the raw maps at the valid pixels, 0 at every other."""
    ok = valid_kitti(disp1, disp2, flow)
    return np.where(ok, disp1, 0).astype(np.uint16), np.where(ok, disp2, 0).astype(np.uint16), \
        np.where(ok[..., None], flow, 0).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ scenes
#: a camera whose projection is exact in float32: with Z = 2, u = X and v = Y for every float (X * 2 and / 2 are exact)
EXACT_CAMERA = (2.0, 0.0, 0.0, 0.0, 0.0, 0.0)
#: KITTI-like, with the three constants that a P_rect_02 carries
KITTI_CAMERA = (-721.5377, 609.5593, 172.854, 44.85728, 0.2163791, 0.002745884)


def exact_points(us, vs, z=2.0):
    """Points that EXACT_CAMERA projects to exactly (u, v), z a power of two: [n, 3] float32."""
    us, vs = np.asarray(us, dtype=f32), np.asarray(vs, dtype=f32)
    s = f32(z) / f32(2)
    return np.stack([us * s, vs * s, np.full(len(us), z, f32)], axis=1).astype(f32)


def back_project(u, v, z, camera):
    """Points that project near (u, v) at depth zc = z (float64 inverse, rounded once: not exact, for random scenes)."""
    f, cx, cy, kx, ky, kz = (float(c) for c in camera)
    u, v, z = (np.asarray(a, dtype=np.float64) for a in (u, v, z))
    Z = z - kz
    return np.stack([(u * z - cx * Z - kx) / f, (v * z - cy * Z - ky) / f, Z], axis=1).astype(f32)


def random_cloud(rng, n, H, W, camera=KITTI_CAMERA, margin=3.0, zlo=2.0, zhi=60.0, bad=0.0):
    """n points scattered over the image and `margin` pixels around it; bad: the share replaced by points that must not project
    (non-finite coordinates, depths at or behind the camera)."""
    u = rng.uniform(-margin, W + margin, n)
    v = rng.uniform(-margin, H + margin, n)
    pc = back_project(u, v, rng.uniform(zlo, zhi, n), camera)
    k = int(bad * n)
    if k:
        rows = rng.choice(n, k, replace=False)
        pc[rows, rng.randint(0, 3, k)] = rng.choice(np.array([np.nan, np.inf, -np.inf, -5.0, 0.0], f32), k)
    return pc


def two_walls(rng, H, W, camera=KITTI_CAMERA, z_front=5.0, z_back=9.0, per_pixel=1.0):
    """A wall over the left two thirds of the image in front of a wall over the whole image: (pc [n, 3], is_front [n])."""
    nb = int(per_pixel * H * W)
    nf = int(per_pixel * H * W * 2 / 3)
    back = back_project(rng.uniform(0, W - 1, nb), rng.uniform(0, H - 1, nb), np.full(nb, z_back), camera)
    front = back_project(rng.uniform(0, (W - 1) * 2 / 3, nf), rng.uniform(0, H - 1, nf), np.full(nf, z_front), camera)
    pc = np.concatenate([back, front])
    is_front = np.concatenate([np.zeros(nb, bool), np.ones(nf, bool)])
    order = rng.permutation(len(pc))
    return pc[order], is_front[order]


def pack(clouds):
    """[n_b, 3] clouds -> ((3, N) float32, prefix list)."""
    prefix = [0]
    for c in clouds:
        prefix.append(prefix[-1] + len(c))
    cat = np.concatenate([np.asarray(c, dtype=f32).reshape(-1, 3) for c in clouds]) if clouds else np.zeros((0, 3), f32)
    return np.ascontiguousarray(cat.T), prefix


def render_batch(clouds, cameras, sizes, attrs=None, **kw):
    """The packed outputs of a batch from render_maps per cloud: dict of pixel_of (N), winner (M), depth (M), attr_map (C, M) or
    None, visible (N), stats (B, 4)."""
    res = [render_maps(c, cam, H, W, None if attrs is None else attrs[b], **kw)
           for b, (c, cam, (H, W)) in enumerate(zip(clouds, cameras, sizes))]
    out = {k: np.concatenate([r[k] for r in res]) for k in ('pixel_of', 'winner', 'depth', 'visible')}
    out['attr_map'] = None if attrs is None else np.concatenate([r['attr_map'] for r in res], axis=1)
    out['stats'] = np.stack([r['stats'] for r in res])
    return out
