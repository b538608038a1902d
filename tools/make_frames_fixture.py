"""Generate tests/golden/frames.npz: small synthetic raw frames and what the REFERENCE's back-projection computes for them.

Runs only where the read-only reference exists (tools/ref_import.py: REF).  The reference's own functions are imported and
called -- kitti_utils.disp_2_depth and pixel2xyz, flyingthings3d_utils.pixel2pc and next_pixel2pc --; nothing of them is
restated here.  kitti_utils imports `png` (pypng) at load time; an empty in-memory module stands in, the way ref_import.py
shims numba: the two functions taken from it never touch it.  Their arguments are prepared from the raw values by this
project's own code, following the definition in include/hpl_bcl.h (a raw disparity r is the disparity r / 256 and is valid
when r > 0; a raw flow value u is the displacement (u - 32768) / 64 and counts when the mask is 1; the second cloud is looked
up at the displaced pixel); the masks select the rows in pixel order, as a boolean index does.

The file is data only: inputs (raw values, calibrations by name) and the reference functions' outputs.

    python tools/make_frames_fixture.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from ref_import import REF  # noqa: E402
import frames_oracle as fo  # noqa: E402

sys.modules.setdefault('png', types.ModuleType('png'))
sys.path.insert(0, os.path.join(REF, 'data_preprocess'))
import flyingthings3d_utils as ref_ft3d_utils  # noqa: E402
import kitti_utils as ref_kitti_utils  # noqa: E402

KITTI_SHAPES = ((37, 131), (5, 64), (40, 140))
FT3D_SHAPES = ((23, 65), (40, 140))
F32 = np.float32


def kitti_by_reference(raw1, raw2, raw_flow, P):
    """The two clouds of a frame through the reference's disp_2_depth and pixel2xyz."""
    H, W = raw1.shape
    ok1, ok2, ok_flow = raw1 > 0, raw2 > 0, raw_flow[..., 2] == 1
    keep = ok1 & ok2 & ok_flow
    depths = []
    for raw, ok in ((raw1, ok1), (raw2, ok2)):
        disparity = np.where(ok, raw.astype(F32) / F32(256), F32(-1)).astype(F32)
        depths.append(ref_kitti_utils.disp_2_depth(disparity, ok, P[0, 0]))
    cols, rows = fo._grid(H, W)
    shift = (raw_flow[..., :2].astype(F32) - F32(32768)) / F32(64)
    px2 = np.where(keep, cols + shift[..., 0], F32(0)).astype(F32)
    py2 = np.where(keep, rows + shift[..., 1], F32(0)).astype(F32)
    pc1 = ref_kitti_utils.pixel2xyz(depths[0], P)
    pc2 = ref_kitti_utils.pixel2xyz(depths[1], P, px=px2, py=py2)
    return pc1[keep], pc2[keep]


def ft3d_by_reference(disp, dchange, flow, occ1, occ2, near):
    """The two clouds of a frame through the reference's pixel2pc and next_pixel2pc; near: None or the cut."""
    pc1 = ref_ft3d_utils.pixel2pc(disp)
    pc2 = ref_ft3d_utils.next_pixel2pc(flow, disp + dchange)
    keep = (occ1 == 0) & (occ2 == 0)
    if near is not None:
        keep &= (pc1[..., 2] > near) & (pc2[..., 2] > near)
    return pc1[keep], pc2[keep]


def main():
    rng = np.random.RandomState(20250)
    out = {}
    with np.errstate(all='ignore'):
        for k, ((H, W), name) in enumerate(zip(KITTI_SHAPES, fo.CALIB_NAMES)):
            d1, d2, fl = fo.kitti_raw(rng, H, W, extreme=k == 1)
            pc1, pc2 = kitti_by_reference(d1, d2, fl, fo.read_P(name))
            assert pc1.dtype == F32 and pc2.dtype == F32 and len(pc1) > 0
            out.update({'kitti%d_disp1' % k: d1, 'kitti%d_disp2' % k: d2, 'kitti%d_flow' % k: fl, 'kitti%d_calib' % k: np.array(name),
                        'kitti%d_pc1' % k: pc1, 'kitti%d_pc2' % k: pc2})
        for k, (H, W) in enumerate(FT3D_SHAPES):
            frame = fo.ft3d_raw(rng, H, W, extreme=k == 0)
            for key, x in zip(('disp', 'dchange', 'flow', 'occ1', 'occ2'), frame):
                out['ft3d%d_%s' % (k, key)] = x
            for tag, near in (('all', None), ('near', -35.)):
                pc1, pc2 = ft3d_by_reference(*frame, near=near)
                assert pc1.dtype == F32 and pc2.dtype == F32 and len(pc1) > 0
                out['ft3d%d_%s_pc1' % (k, tag)], out['ft3d%d_%s_pc2' % (k, tag)] = pc1, pc2
    path = os.path.join(ROOT, 'tests', 'golden', 'frames.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
