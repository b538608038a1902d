"""numpy restatement of hpl_lattice_query (include/hpl_bcl.h) over the C oracle's keys: the tests' oracle for dense-flow
queries (tests/test_gpu_dense_flow.py; its self-check in tests/test_dense_flow_cpu.py)."""
import numpy as np

from hplflownet_amd.synthetic import SCALES_FILTER_MAP


def np_pack(k, mm):
    res = 0
    for i in range(3):
        res += int(k[i]) - int(mm[i])
        res *= int(mm[4 + i + 1]) - int(mm[i + 1]) + 1
    return res + int(k[3]) - int(mm[3])


class NpQuery(object):
    """numpy restatement of hpl_lattice_query for one pair: the oracle's keys of both clouds give the level's key range, pc1's
    keys and level-0 offsets (generate_data) the vertex dict."""

    def __init__(self, pc1, pc2, scale=SCALES_FILTER_MAP[0][0]):
        from oracle import lattice_oracle as LO
        self.LO, self.scale = LO, np.float32(scale)
        k1, _, _ = LO.keys_and_barycentric(pc1 * self.scale)
        k2, _, _ = LO.keys_and_barycentric(pc2 * self.scale)
        self.mm = np.array([min(k1[x].min(), k2[x].min()) for x in range(4)] + [max(k1[x].max(), k2[x].max()) for x in range(4)])
        gd = LO.generate_data(pc1.T, pc2.T, SCALES_FILTER_MAP[:1])[0]
        off = gd['pc1_lattice_offset']
        self.ids = {}
        for n in range(pc1.shape[1]):
            for r in range(4):
                self.ids[tuple(int(v) for v in k1[:, n, r])] = int(off[r, n])
        self.packed = {np_pack(k, self.mm) for k in self.ids}

    def __call__(self, q, renorm):
        keys, w, _ = self.LO.keys_and_barycentric(np.ascontiguousarray(q, np.float32) * self.scale)
        Q = q.shape[1]
        off = np.zeros((4, Q), np.int32)
        bary = np.zeros((4, Q), np.float32)
        cov = np.zeros(Q, np.float32)
        aliased = np.zeros(Q, bool)
        for i in range(Q):
            ids, full, c = [], True, np.float32(0)
            for r in range(4):
                k = tuple(int(v) for v in keys[:, i, r])
                inr = all(self.mm[x] <= k[x] <= self.mm[4 + x] for x in range(4))
                v = self.ids.get(k, -1) if inr else -1
                if not inr and np_pack(k, self.mm) in self.packed:
                    aliased[i] = True
                ids.append(v)
                if v >= 0:
                    c = np.float32(c + w[r, i])
                elif w[r, i] != 0:
                    full = False
            if full:
                c = np.float32(1)
            for r in range(4):
                wr = w[r, i] if ids[r] >= 0 else np.float32(0)
                if renorm and not full and c > 0:
                    wr = np.float32(wr / c)
                bary[r, i] = wr
                off[r, i] = max(ids[r], 0)
            cov[i] = c
        return off, bary, cov, aliased
