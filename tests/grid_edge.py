"""The cloud of the grid-edge tests (csrc/grid_common.h): at radius or max_dist 1.0 the cell edge is 1.001 and
the last cells the key's 19-bit fields can hold are +-(2^18 - 2).  Per axis and sign, four points in that last cell and four in
the cell one further out, a quarter of a metre across the border from them: the inner ones are neighbours of each other and of
nobody else, the outer ones take no part although they lie within the radius of the inner ones.  Every coordinate is a
multiple of 1/32, exact in float32 at 2^18."""
import numpy as np

from icp_oracle import CELL_MARGIN, CELL_MAX

EDGE = CELL_MAX                                  # 262 142
#: the last float32 multiples of 1/4 inside cell +EDGE and cell -EDGE, and the first ones outside
IN_HI, OUT_HI, IN_LO, OUT_LO = 262405.0, 262405.25, -262404.0, -262404.25
SPREAD = np.array([[0.0, 0.125, 0.25, 0.375],    # along the axis, away from the border
                   [0.0, 0.25, 0.0, 0.25],
                   [0.0, 0.0, 0.25, 0.125]])
REST = (0.5, 4.5)                                # the other two coordinates start here (cells 0 and 4)


def cell(x, radius=1.0):
    """The restatement's cell of float32 coordinates (tests/icp_oracle.in_range)."""
    inv_cell = 1.0 / (CELL_MARGIN * np.float64(np.float32(radius)))
    return np.floor(np.asarray(x, np.float32).astype(np.float64) * inv_cell)


def cloud():
    """-> (pc (3, 48) float32, inside (48,) bool, cluster (48,) int): cluster 4 a + 2 s + o of axis a, sign s (0: +, 1: -) and
    o = 1 for the cell one further out."""
    pts, inside, cluster = [], [], []
    for a in range(3):
        for s, (start_in, start_out) in enumerate(((IN_HI, OUT_HI), (IN_LO, OUT_LO))):
            sign = 1.0 if s == 0 else -1.0
            for o, start in enumerate((start_in, start_out)):
                p = np.empty((3, 4))
                p[a] = start + sign * (1.0 if o else -1.0) * SPREAD[0]
                p[(a + 1) % 3] = REST[0] + SPREAD[1]
                p[(a + 2) % 3] = REST[1] + SPREAD[2]
                pts.append(p)
                inside += [o == 0] * 4
                cluster += [4 * a + 2 * s + o] * 4
    pc = np.concatenate(pts, 1)
    assert np.array_equal(pc.astype(np.float32).astype(np.float64), pc)         # exact in float32
    return pc.astype(np.float32), np.array(inside), np.array(cluster)


def check_cells(pc, inside, cluster):
    """The restatement puts every chosen coordinate in the cell it is meant for."""
    c = cell(pc)
    for j in range(pc.shape[1]):
        a, s, o = cluster[j] // 4, cluster[j] // 2 % 2, cluster[j] % 2
        want = (EDGE + o) * (1 if s == 0 else -1)
        assert c[a, j] == want, (j, c[:, j], want)
        assert c[(a + 1) % 3, j] == 0 and c[(a + 2) % 3, j] == 4
        assert inside[j] == (o == 0) == bool((np.abs(c[:, j]) <= CELL_MAX).all())
