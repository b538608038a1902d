"""hplflownet_amd -- MI355X-native bilateral-convolution hot path of HPLFlowNet.

Public surface (mirrors the reference's operator interface for the path):
    BilateralConvFlex, BilateralCorrelationFlex, sparse_sum     (layers; bcl.py)
    GenerateDataUnsymmetric                                      (GPU lattice; lattice.py)
    HPLFlowNet, HPLFlowNetShallow, DeviceLattice, DenseFlow      (callers; flownet.py)
    rigid_refine                                                 (rigid motion from flow; flownet.py, ops.rigid_fit)
    icp_register                                                 (rigid registration of a cloud pair; flownet.py, ops.icp)
    estimate_normals                                             (surface normals of clouds; flownet.py, ops.normals)
    segment_motion                                               (moving objects from flow; flownet.py, ops.motion_segment)
    piecewise_rigid                                              (ego-motion + a rigid motion per object; flownet.py, ops.object_fit)
    selfsup_loss                                                 (Chamfer + smoothness loss; flownet.py, ops.selfsup_loss)
    remove_ground                                                (fitted-plane ground removal; flownet.py, ops.ground_fit)
    remove_outliers                                              (statistical / radius outlier removal; flownet.py, ops.outlier_filter)
    voxel_downsample                                             (voxel-grid downsampling; flownet.py, ops.voxel_downsample)
    fps_sample                                                   (farthest point sampling; flownet.py, ops.fps)
    frames_from_kitti, frames_from_ft3d                          (clouds from raw disparity / flow maps; flownet.py, ops.frames_from_*)
    render_maps, visibility, flow_to_kitti_maps                  (maps from clouds: z-buffer, visibility, KITTI's PNG values;
                                                                  flownet.py, ops.render_maps, ops.maps_to_kitti)
The arithmetic lives in libhplbcl.so (csrc/*.hip, C ABI in include/hpl_bcl.h).
"""
from .bcl import (BilateralConvFlex, BilateralCorrelationFlex, Conv1dReLU, Conv2dReLU, Conv3dReLU,  # noqa: F401
                  sparse_sum)
from .flownet import (DenseFlow, DeviceLattice, HPLFlowNet, HPLFlowNetShallow, estimate_normals, flow_to_kitti_maps, fps_sample,  # noqa: F401
                      frames_from_ft3d, frames_from_kitti, icp_register, piecewise_rigid, remove_ground, remove_outliers, rigid_refine, segment_motion,
                      render_maps, selfsup_loss, visibility,
                      voxel_downsample)
from .lattice import GenerateDataUnsymmetric, to_reference_format  # noqa: F401

__version__ = '0.1.0'
