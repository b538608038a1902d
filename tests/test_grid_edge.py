"""CPU: the cloud of the grid-edge GPU tests (tests/grid_edge.py) lies where it is meant to, by the restatements' own cell rule,
and the restatements give it the outcome the GPU tests then demand of the device."""
import numpy as np

import grid_edge as E
import icp_oracle as IO
import normals_oracle as NO


def test_every_coordinate_lies_in_the_cell_it_is_meant_for():
    pc, inside, cluster = E.cloud()
    assert pc.shape == (3, 48) and pc.dtype == np.float32 and inside.sum() == 24
    E.check_cells(pc, inside, cluster)
    assert np.array_equal(IO.in_range(pc, 1.0), inside)
    # the float32 steps around the borders: the cell changes exactly where the cloud says it does
    for inner, outer in ((E.IN_HI, E.OUT_HI), (E.IN_LO, E.OUT_LO)):
        assert abs(E.cell(np.float32(inner))) == E.EDGE and abs(E.cell(np.float32(outer))) == E.EDGE + 1
        assert abs(outer - inner) == 0.25


def test_the_restatements_keep_the_edges_apart():
    pc, inside, cluster = E.cloud()
    count, nbr, nd2 = NO.neighbourhoods(pc, 8, 1.0)
    assert (count[inside] == 4).all() and (count[~inside] == 0).all()
    for j in np.flatnonzero(inside):
        assert (cluster[nbr[j, :4]] == cluster[j]).all() and (nbr[j, 4:] == -1).all()
    # without the range rule the outer points would be neighbours: they lie within the radius of the inner ones
    d = pc[:, :, None].astype(np.float64) - pc[:, None, :].astype(np.float64)
    near = (d * d).sum(0) <= 1.0
    assert all(near[j][~inside].any() for j in np.flatnonzero(inside))
    src = pc + np.float32(0.0625)
    E.check_cells(src, inside, cluster)
    match, dist2 = IO.match(src, pc, *IO.IDENTITY, 1.0)
    assert (match[~inside] == -1).all() and np.isinf(dist2[~inside]).all()
    assert (match[inside] >= 0).all() and (cluster[match[inside]] == cluster[inside]).all()
