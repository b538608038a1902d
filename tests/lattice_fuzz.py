"""Hard clouds for the lattice builders, the size of their key ranges, and the comparison with the C oracle, stated once
for the tests that fuzz the builders (tests/test_lattice_fuzz_cpu.py, tests/test_gpu_lattice_fuzz.py and
test_device_lattice_fuzz_vs_oracle of tests/test_gpu_layers.py).  A helper module: it holds no test and no fixture."""
import math

import numpy as np

from hplflownet_amd.synthetic import SCALES_FILTER_MAP

#: the kinds test_device_lattice_fuzz_vs_oracle has always drawn from (their draws and formulas are unchanged)
OLD_KINDS = ('cloud', 'dup', 'line', 'plane', 'far', 'tiny')
NEW_KINDS = ('axis', 'same', 'far32', 'far64', 'outlier', 'lopsided')
KINDS = OLD_KINDS + NEW_KINDS

#: (n1, n2) every kind is checked at: the smallest pair, a lopsided one, around a wave of 64 points, more than one workgroup
SIZES = ((1, 1), (2, 300), (63, 65), (300, 257))

#: log2 of the level-0 key range 'far32' / 'far64' are stretched to.  The plain base cloud has 2^31.9 keys at n = 300, x32
#: and x64 of it 2^51.9 and 2^55.9, and a pair of two points far fewer, so the multiplier is solved for from the cloud's own
#: extent (n = 300: x74 and x136; two points: whatever brings them that far apart).  far32 is 0.6 bits under the 57 a batch
#: of 64 leaves a pair; far64 lies between the 59 bits of a batch of 16 and the 61 of a batch of 4, more than half a bit from
#: both, and a tenth of a bit under the 60 of a batch of 5.
FAR_BITS = {'far32': 56.4, 'far64': 59.9}
#: where 'outlier' puts pc1[0]: (t, -t, t).  2^60.2 keys at every size (t = 2000 gives 2^55.9).
OUTLIER_AT = 4200.0


def pair_bits(B):
    """bits below the pair digit of a batch of B pairs (csrc/lattice_fused.hip, pair_shift): B = 2: 62, B = 64: 57"""
    assert B >= 2
    return 63 - (B - 1).bit_length()


def _elevate():
    """the (4, 3) elevation matrix of the permutohedral lattice times its standard deviation, in float64"""
    E = np.zeros((4, 3))
    for i in range(4):
        for j in range(3):
            left = (1.0 if j >= i else 0.0) - (i if (i >= 1 and j == i - 1) else 0.0)
            E[i, j] = left / math.sqrt((j + 1) * (j + 2))
    return E * (4 * math.sqrt(2.0 / 3.0))


def _stretch(p1, p2, bits):
    """the multiplier that brings the level-0 key range of the pair to 2^bits: the keys of a point lie within 4 of its
    elevated position, so the range of coordinate i is the cloud's elevated extent w_i times the multiplier, plus a few keys"""
    e = np.concatenate([p1, p2]).astype(np.float64) @ _elevate().T * float(SCALES_FILTER_MAP[0][0])
    w = e.max(0) - e.min(0)
    lo, hi = 1.0, 2.0 ** 40
    for _ in range(200):
        mid = math.sqrt(lo * hi)
        if sum(math.log2(mid * x + 6.0) for x in w) < bits:
            lo = mid
        else:
            hi = mid
    return np.float32(lo)


def fuzz_pair(kind, n1, n2, seed):
    """-> (pc1 (n1, 3), pc2 (n2, 3)) float32, deterministic from the seed.  The base cloud: x, y in +-8, z in 1.5 .. 35.
      cloud     the base cloud                            dup       few distinct points, pc2 starts as a copy of pc1
      line      pc1 on the z axis, pc2 parallel to x      plane     pc1 in z = 10, pc2 in x = -1
      far       x40 (2^53.1 keys at n = 300)              tiny      x1e-3: inside one simplex at every level
      axis      all points on one coordinate axis (seed % 3), both signs, every third exactly 0: ties in the rank sort
      same      all points of both clouds at one position, (0, 0, z)
      far32     stretched to 2^56.4 keys (FAR_BITS)        far64     stretched to 2^59.9 keys
      outlier   the base cloud with pc1[0] at OUTLIER_AT x (1, -1, 1)
      lopsided  n1 points against ONE (n2 is ignored)"""
    assert kind in KINDS, kind
    if kind == 'lopsided':
        n2 = 1
    rng = np.random.RandomState(seed)
    p1 = rng.uniform(-8, 8, (n1, 3)).astype(np.float32)
    p1[:, 2] = rng.uniform(1.5, 35, n1)
    p2 = rng.uniform(-8, 8, (n2, 3)).astype(np.float32)
    p2[:, 2] = rng.uniform(1.5, 35, n2)
    if kind == 'dup':
        p1[:] = p1[rng.randint(0, max(1, n1 // 4), n1)]
        p2[: min(n1, n2)] = p1[: min(n1, n2)]
    elif kind == 'line':
        p1[:, :2] = 0.0
        p2[:, 1:] = p2[0, 1:]
    elif kind == 'plane':
        p1[:, 2] = 10.0
        p2[:, 0] = -1.0
    elif kind == 'far':
        p1 *= 40.0
        p2 *= 40.0
    elif kind == 'tiny':
        p1 *= 1e-3
        p2 *= 1e-3
    elif kind == 'axis':
        ax = seed % 3
        for p in (p1, p2):
            v = p[:, 0].copy()              # +-8
            v[1::3] = 0.0
            p[:] = 0.0
            p[:, ax] = v
    elif kind == 'same':
        p1[:] = (0.0, 0.0, p1[0, 2])        # on the z axis: three of a point's four elevated residuals tie as well
        p2[:] = p1[0]
    elif kind in FAR_BITS:
        m = _stretch(p1, p2, FAR_BITS[kind])
        p1 *= m
        p2 *= m
    elif kind == 'outlier':
        p1[0] = (OUTLIER_AT, -OUTLIER_AT, OUTLIER_AT)
    return p1, p2


def _walk(pc1, pc2):
    """the levels as oracle.lattice_oracle.generate_data walks them: yields (keys1, keys2, emg1, emg2, level tables)"""
    from oracle import lattice_oracle as LO
    L = LO.lib()
    last1 = np.ascontiguousarray(pc1.T, dtype=np.float32).copy()
    last2 = np.ascontiguousarray(pc2.T, dtype=np.float32).copy()
    n = len(SCALES_FILTER_MAP)
    for idx, (scale, bcn_r, cf_r, cc_r) in enumerate(SCALES_FILTER_MAP):
        last1 = last1 * np.float32(scale)
        last2 = last2 * np.float32(scale)
        k1, _, e1 = LO.keys_and_barycentric(last1)
        k2, _, e2 = LO.keys_and_barycentric(last2)
        lev = LO.build_level(k1, k2, (bcn_r, cf_r, cc_r), idx != n - 1)
        yield k1, k2, e1, e2, lev
        if idx != n - 1:
            n1 = np.empty((3, lev['h1']), np.float32)
            n2 = np.empty((3, lev['h2']), np.float32)
            L.hpl_next_level_points(lev['last1'], lev['h1'], float(scale), n1)
            L.hpl_next_level_points(lev['last2'], lev['h2'], float(scale), n2)
            last1, last2 = n1, n2


def survey(pc1, pc2):
    """one walk of the oracle over the pair -> dict(bits: per level log2 of the product of the four per-coordinate key ranges
    over both clouds -- the number of packed keys of the pair, what pair_range of csrc/lattice_fused.hip holds against the
    bits below the pair digit, from the oracle's own keys and in Python integers; verts: per level (H1, H2); ties: a point
    of pc1 has two equal entries in its level-0 el_minus_gr, so its rank sort is decided by the tie rule)"""
    bits, verts, ties = [], [], False
    for idx, (_, _, e1, _, lev) in enumerate(_walk(pc1, pc2)):
        R = 1
        for lo, hi in zip(lev['key_mins'].tolist(), lev['key_maxs'].tolist()):
            R *= int(hi) - int(lo) + 1
        bits.append(math.log2(R))
        verts.append((lev['h1'], lev['h2']))
        if idx == 0:
            ties = any(len(set(e1[:, p].tolist())) < 4 for p in range(e1.shape[1]))
    return dict(bits=bits, verts=verts, ties=ties)


def range_bits(pc1, pc2):
    """per level: log2 of the number of packed keys of the pair (survey()['bits'])"""
    return survey(pc1, pc2)['bits']


def default_bound(n1, n2):
    """vertices per cloud and level a fused build takes without a rebuild before it has seen a pair (default_row_cap of
    csrc/lattice_fused.hip): what `fallbacks == 0` on a first build assumes of its input"""
    return 18 * max(n1, n2) + 64


#: test_tight_bounds_after_a_degenerate_pair: the kinds one fused builder sees in turn, and their (n1, n2, seed)
TIGHT_KINDS = ('tiny', 'cloud', 'far32', 'same')
TIGHT_CASE = (300, 257, 1)


def overflowing_levels(bounds, verts, n1, n2):
    """levels at which a pair of `verts` [(H1, H2)] vertices outgrows the per-level bounds in force (0: the default)"""
    return [L for L, v in enumerate(verts) if max(v) > (bounds[L] if bounds[L] > 0 else default_bound(n1, n2))]


_ORACLE = {}


def oracle_pair(kind, n1, n2, seed):
    """-> (pc1, pc2, generate_data of the C oracle over all 7 scales), computed once per case and shared: read only"""
    from oracle import lattice_oracle as LO
    key = (kind, n1, n2, seed)
    if key not in _ORACLE:
        pc1, pc2 = fuzz_pair(kind, n1, n2, seed)
        _ORACLE[key] = (pc1, pc2, LO.generate_data(pc1, pc2, SCALES_FILTER_MAP))
    return _ORACLE[key]


def assert_equals_oracle(lat, pc1, pc2, what='', gd=None):
    """every key of every level of the reference wire format of `lat` == the C oracle's generate_data over (pc1, pc2),
    bit for bit.  gd: that generate_data if the caller has it already.  -> gd"""
    import torch
    import hplflownet_amd as H
    from oracle import lattice_oracle as LO
    if gd is None:
        gd = LO.generate_data(pc1, pc2, SCALES_FILTER_MAP)
    ref = H.to_reference_format(lat)
    assert len(ref) == len(gd), what
    for L, (x, d) in enumerate(zip(ref, gd)):
        for k, v in d.items():
            got = x[k].cpu().numpy() if torch.is_tensor(x[k]) else x[k]
            assert np.array_equal(np.asarray(got).reshape(-1), np.asarray(v).reshape(-1)), (what, L, k)
    return gd
