"""torch_points3d_amd -- MI355X-native implementation of torch-points3d's data-parallel hot path.

`torch_points3d_amd.torchpoints` serves the `torch_points_kernels` function API from hand-written HIP
kernels (libtp3d_hip.so, C-ABI in include/tp3d_hip.h); `torch_points3d_amd.dense` / `.pointnet2` are the
host-side mirror of the reference's dense PointNet++ modules that call it; `.pointnet2_mp` is the message-passing
PointNet++ (ragged batches: FPSSampler, SAModule, GlobalBaseModule, FPModule, PointNet2MP).
"""
from .torchpoints import (  # noqa: F401
    ball_query,
    fps_quota,
    fps_ragged,
    furthest_point_sample,
    grouping_operation,
    three_interpolate,
    three_nn,
)
from .pointnet2_mp import (  # noqa: F401
    FPModule,
    FPSSampler,
    GlobalBaseModule,
    MultiscaleRadiusNeighbourFinder,
    PointConv,
    PointNet2MP,
    RadiusNeighbourFinder,
    SAModule,
)
from .pvcnn import (  # noqa: F401  (the factory `pvcnn.pvcnn` stays in its module: the name is the module's)
    PVCNN,
    PointTensor,
    initial_voxelize,
    point_to_voxel,
    voxel_to_point,
)

__version__ = "0.1.0"
