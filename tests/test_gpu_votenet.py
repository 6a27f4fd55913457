"""VoteNet (torch_points3d_amd/votenet.py) on the HIP kernels against tests/golden/votenet.npz: the reference's own
VotingModule, ProposalModule, VoteNetResults and get_loss over its PointNetMSGDown / DenseFPModule and the CPU oracle
kernels (tests/golden/make_golden_votenet.py), the VoteNetPaper layout reduced to B = 2, N = 512, FEAT = 1, npoint
128 / 64 / 32 / 16, nsample 16 / 8 / 8 / 8, in_feat 8, 64 seeds, 16 proposals, 4 classes and size clusters, one heading bin.

Bars (tests/votenet_cases.py; the ones every family here uses): teacher-forced stages rtol 1e-5 with atol 1e-5 or twice
the reference pass's own distance to its float64 evaluation; the chained training pass by its distance to the stored
float64 pass (<= 4x max, 2x RMS of the reference pass's own); objectness_label, objectness_mask and object_assignment
exactly; every loss term against its float64 value (1e-5 relative, or 4x the reference's own fp32 distance); parameter
gradients by relative L2 against the float64 gradients, <= max(1e-4, 4x the reference's own fp32-to-fp64 distance stored
in the fixture: at most 6.5e-5); eval mode 1e-5 * scale.  None of these figures comes from the code under test."""
import pytest
import torch

import votenet_cases as vc
from golden_util import report
from torch_points3d_amd.dense import Data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return vc.net_gold()


def test_stages_teacher_forced_on_the_fixture(gold):
    vc.check_stages_teacher_forced(gold, vc.build_net(gold, DEV), DEV)


def test_chained_pass_assignments_losses_gradients_buffers_and_eval(gold):
    vc.check_chained_pass(gold, vc.build_net(gold, DEV), DEV, report=report)


def test_backbone_without_sampling_ids_samples_the_feature_positions(gold, hip):
    """any module with output_nc and a dense forward serves as backbone; without sampling_id_0 the seeds come from
    furthest point sampling of the feature positions"""
    net = vc.build_net(gold, DEV)

    class Bare(torch.nn.Module):
        output_nc = 32

        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, data):
            out = self.inner(data)
            return Data(pos=out.pos, x=out.x)

    net.backbone_model = Bare(net.backbone_model)
    net._num_seeds = 48
    net.eval()
    with torch.no_grad():
        res = net(Data(pos=gold["pos"].to(DEV), x=gold["x"].to(DEV)))
    want = hip.furthest_point_sample(gold["down1_pos"].to(DEV), 48)
    assert torch.equal(res.seed_inds, want) and tuple(res.seed_pos.shape) == (2, 48, 3)
    assert torch.equal(res.seed_pos, gold["down1_pos"].to(DEV).gather(1, want.unsqueeze(-1).expand(-1, -1, 3)))
    assert tuple(res.center.shape) == (2, 16, 3) and bool(torch.isfinite(res.center).all())
