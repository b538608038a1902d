"""Write the processed tree of a raw download: what the reference's data_preprocess/process_kitti.py and
process_flyingthings3d_subset.py write, computed on the device (flownet.frames_from_kitti / frames_from_ft3d).

    python tools/preprocess.py RAW OUT --dataset KITTI --kitti-calib DIR
        RAW/training/{disp_occ_0,disp_occ_1,flow_occ}/NNNNNN_10.png -> OUT/NNNNNN/{pc1,pc2}.npy
        (data.KITTI reads OUT = <data_root>/KITTI_processed_occ_final)
    python tools/preprocess.py RAW OUT --dataset FlyingThings3DSubset [--near -35 | --no-near]
        RAW/{train,val}/... -> OUT/{train,val}/<name>/{pc1,pc2}.npy
        (data.FlyingThings3DSubset reads OUT = <data_root>/FlyingThings3D_subset_processed_35m)

Every file is an [n, 3] float32 array, bit for bit the reference's.  --batch frames go through one device call.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hplflownet_amd import data, flownet  # noqa: E402


def _save(out_dir, pc1, pc2):
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, 'pc1.npy'), np.ascontiguousarray(pc1.t().cpu().numpy()))
    np.save(os.path.join(out_dir, 'pc2.npy'), np.ascontiguousarray(pc2.t().cpu().numpy()))


def _batches(items, n):
    for at in range(0, len(items), n):
        yield items[at:at + n]


def kitti(raw, out, calib, batch, device):
    root = os.path.join(raw, 'training')
    names = [nm[:-3] for nm in data._listed(os.path.join(root, 'disp_occ_0'), '.png') if nm.endswith('_10')]
    for group in _batches(names, batch):
        frames = [data.read_kitti_raw_frame(raw, nm) + (data.read_kitti_P(os.path.join(calib, nm + '.txt')),) for nm in group]
        pc1, pc2 = flownet.frames_from_kitti(frames, device=device)[:2]
        for nm, a, b in zip(group, pc1, pc2):
            _save(os.path.join(out, nm), a, b)
    return len(names)


def ft3d(raw, out, near, batch, device):
    total = 0
    lead, ext = data.FT3D_RAW_LAYOUT[2]
    for split in ('train', 'val'):
        root = os.path.join(raw, split)
        if not os.path.isdir(root):
            continue
        names = data._listed(os.path.join(root, *lead), ext)
        for group in _batches(names, batch):
            pc1, pc2 = flownet.frames_from_ft3d([data.read_ft3d_raw_frame(root, nm) for nm in group], near=near, device=device)[:2]
            for nm, a, b in zip(group, pc1, pc2):
                _save(os.path.join(out, split, nm), a, b)
        total += len(names)
    return total


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('raw')
    ap.add_argument('out')
    ap.add_argument('--dataset', required=True, choices=['KITTI', 'FlyingThings3DSubset'])
    ap.add_argument('--kitti-calib', default=None, metavar='DIR', help='KITTI: the directory of the calib_cam_to_cam files (NNNNNN.txt)')
    ap.add_argument('--near', type=float, default=-35.0, help='FlyingThings3DSubset: the near cut of --only_save_near_pts (default -35)')
    ap.add_argument('--no-near', action='store_true', help='FlyingThings3DSubset: keep every visible correspondence')
    ap.add_argument('--batch', type=int, default=16, help='frames per device call (1 .. 64, default 16)')
    ap.add_argument('--device', default='cuda')
    a = ap.parse_args(argv)
    if not 1 <= a.batch <= 64:
        ap.error('--batch takes 1 .. 64')
    if a.dataset == 'KITTI':
        if a.kitti_calib is None or not os.path.isdir(a.kitti_calib):
            ap.error('--dataset KITTI needs --kitti-calib DIR')
        n = kitti(a.raw, a.out, a.kitti_calib, a.batch, a.device)
    else:
        n = ft3d(a.raw, a.out, None if a.no_near else a.near, a.batch, a.device)
    print('%d frames -> %s' % (n, a.out))
    return n


if __name__ == '__main__':
    main()
