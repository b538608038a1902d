"""GPU: every row of tests/refusals.py is refused by the one it names, with a text that names the argument, and every good
call runs.  Nothing here launches more than the good calls."""
import pytest
import torch

import refusals

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('op_row', refusals.ROWS, ids=refusals.row_id)
def test_refused(op_row):
    assert refusals.verdict(op_row[0], op_row[1], 'cuda') is None


@pytest.mark.parametrize('op', refusals.OPS, ids=lambda op: op.name)
def test_good_calls_run(op):
    refusals.run_good_calls(op, 'cuda')
    torch.cuda.synchronize()


def test_empty_batches_launch_nothing_and_return_these():
    """N = 0 with B = 2 (prefix [0, 0, 0]): every op's result against literals, in values, shapes and dtypes."""
    from hplflownet_amd import ops
    f32, i32 = torch.float32, torch.int32
    e3, er, e1 = torch.zeros(3, 0, device='cuda'), torch.zeros(0, 3, device='cuda'), torch.zeros(0, device='cuda')
    pre = [0, 0, 0]
    eye = torch.eye(3, device='cuda').expand(2, 3, 3)

    def has(t, shape, dtype, value=None):
        return tuple(t.shape) == shape and t.dtype == dtype and (value is None or bool((t == value).all()))

    R, t, stats, refined, residual = ops.rigid_fit(e3, er, prefix=pre, return_residual=True)
    assert torch.equal(R, eye) and R.dtype == f32 and has(t, (2, 3), f32, 0) and has(stats, (2, 4), f32, 0)
    assert has(refined, (0, 3), f32) and has(residual, (0,), f32)
    R, t, stats, flow, match, dist2 = ops.icp(e3, e3, src_prefix=pre, dst_prefix=pre, return_matches=True)
    assert torch.equal(R, eye) and has(t, (2, 3), f32, 0) and has(stats, (2, 6), f32, 0)
    assert has(flow, (0, 3), f32) and has(match, (0,), i32) and has(dist2, (0,), f32)
    init = (torch.full((2, 3, 3), 2.0, device='cuda'), torch.full((2, 3), 3.0, device='cuda'))
    R, t, stats, _ = ops.icp(e3, torch.zeros(3, 4, device='cuda'), init=init, src_prefix=pre, dst_prefix=[0, 1, 4])
    assert has(R, (2, 3, 3), f32, 2) and has(t, (2, 3), f32, 3) and has(stats, (2, 6), f32, 0)      # init handed back
    plane, stats, ground, keep, votes, height = ops.ground_fit(e3, prefix=pre, hyps=5, return_votes=True, return_height=True)
    assert has(plane, (2, 4), f32, 0) and stats.dtype == i32 and stats.tolist() == [[0, -1, 0, 0]] * 2
    assert has(ground, (0,), torch.uint8) and has(keep, (0,), i32) and has(votes, (2, 5), i32, -1) and has(height, (0,), f32)
    labels, info, motion, stats = ops.motion_segment(e3, er, e1, prefix=pre, max_objects=4)
    assert has(labels, (0,), i32) and info.dtype == i32 and info.tolist() == [[[-1, 0]] * 4] * 2
    assert has(motion, (2, 4, 6), f32, 0) and has(stats, (2, 4), i32, 0)
    out = torch.ones(3, 6, device='cuda')
    out_pc, out_attrs, idx, dist, cover, stats = ops.fps(e3, 3, torch.zeros(2, 0, device='cuda'), prefix=pre, return_cover=True, out=out)
    assert out_pc is out and has(out, (3, 6), f32, 0) and has(out_attrs, (2, 6), f32, 0) and has(idx, (2, 3), i32, -1)
    assert has(dist, (2, 3), f32, 0) and has(cover, (0,), f32) and has(stats, (2, 4), i32, 0)
    assert ops.fps(e3, 3, prefix=pre)[1] is None and ops.fps(e3, 3, prefix=pre)[4] is None
    out_pc, out_attrs, count, rep, voxel_of, stats = ops.voxel_downsample(e3, torch.zeros(2, 0, device='cuda'), prefix=pre)
    assert has(out_pc, (3, 0), f32) and has(out_attrs, (2, 0), f32) and all(has(x, (0,), i32) for x in (count, rep, voxel_of))
    assert has(stats, (2, 4), i32, 0)
    normal, curvature, count, nbr, nbr_d2 = ops.normals(e3, k=4, prefix=pre, return_neighbors=True)
    assert has(normal, (3, 0), f32) and has(curvature, (0,), f32) and has(count, (0,), i32) and has(nbr, (0, 4), i32) and has(nbr_d2, (0, 4), f32)
    loss, dflow, nn12, nn21, nbr = ops.selfsup_loss(e3, er, torch.zeros(3, 4, device='cuda'), k=2, prefix1=pre, prefix2=[0, 1, 4],
                                                    return_neighbors=True)
    assert has(loss, (2, 4), f32, 0) and has(dflow, (0, 3), f32) and has(nn12, (0,), i32) and has(nn21, (4,), i32, -1) and has(nbr, (2, 0), i32)
    assert ops.selfsup_loss(e3, er, e3, prefix1=pre, prefix2=pre, need_grad=False)[1] is None
    res = ops.knn_interpolate(torch.zeros(3, 10, device='cuda'), torch.zeros(10, 2, device='cuda'), e3, return_neighbors=True)     # Q = 0
    assert has(res[0], (0, 2), f32) and has(res[1], (3, 0), i32) and has(res[2], (3, 0), f32)
    torch.cuda.synchronize()
