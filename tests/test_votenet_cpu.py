"""VoteNet without a GPU (torch_points3d_amd/votenet.py): the configuration against the reference's YAML, the three
behaviours of the reference's code that are kept on purpose, the C-ABI of the detection entry points, the reference's
known answers (test/test_boxstuff.py) and fixtures through the numpy path CPU tensors take, and the network over the CPU
oracle kernels against tests/golden/votenet.npz.  Shared checks and their bars: tests/votenet_cases.py."""
import json
import os
import re

import numpy as np
import pytest
import torch

import votenet_cases as vc
from conftest import GOLDEN, ROOT
from torch_points3d_amd import votenet as V
from torch_points3d_amd.dense import Data

CPU = "cpu"


@pytest.fixture(scope="module")
def cfg():
    with open(os.path.join(GOLDEN, "votenet_config.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ configuration
@pytest.mark.parametrize("feat", [0, 1, 3])
def test_config_numbers_are_the_yaml_s(cfg, feat):
    want = cfg["yaml"]["feat%d" % feat]
    got = V.votenet_config("VoteNetPaper", feat, 18, np.ones((18, 3)))
    down, up = want["backbone"]["config"]["down_conv"], want["backbone"]["config"]["up_conv"]
    bb = got["backbone"]
    assert bb["npoint"] == down["npoint"] and bb["radii"] == down["radii"] and bb["nsample"] == down["nsamples"]
    assert bb["down_conv_nn"] == down["down_conv_nn"] and bb["up_conv_nn"] == up["up_conv_nn"]
    assert bb["save_sampling_id"] == down["save_sampling_id"] and bb["normalize_xyz"] == down["normalize_xyz"]
    assert bb["skip"] == up["skip"]
    assert got["voting"]["vote_factor"] == want["voting"]["vote_factor"]
    assert got["voting"]["num_points_to_sample"] == want["voting"]["num_points_to_sample"]
    agg, wagg = got["proposal"]["vote_aggregation"], want["proposal"]["vote_aggregation"]
    for k in ("npoint", "radii", "nsample", "normalize_xyz", "module_name"):
        assert agg[k] == wagg[k], k
    # the file's aggregation widths are replaced by VoteNet2.__init__ (votenet2.py:75-77)
    assert wagg["down_conv_nn"] == [[259, 128, 128, 128]] and agg["down_conv_nn"] == [[259, 256, 256]]
    for k in ("num_class", "num_heading_bin", "num_proposal", "sampling"):
        assert got["proposal"][k] == want["proposal"][k], k
    for k in ("far_threshold", "near_threshold", "gt_vote_factor", "objectness_cls_weights"):
        assert got["loss_params"][k] == want["loss_params"][k], k
    with pytest.raises(ValueError):
        V.votenet_config("VoteNetMink", feat, 18, np.ones((18, 3)))


def test_state_dict_keys_are_the_reference_s(cfg):
    net = V.VoteNet(vc.reduced_config(), feat=1, num_classes=4, mean_size_arr=vc.MEAN_SIZE)
    assert list(net.state_dict().keys()) == cfg["state_dict_keys"]
    full = V.VoteNet("VoteNetPaper", feat=1, num_classes=18, mean_size_arr=np.ones((18, 3)))
    assert full.proposal_cls_module.conv2.out_channels == (256 + 2 + 3 + 2 + 18 * 4 + 18) // 2
    assert full.proposal_cls_module.conv3.out_channels == 97 and full.backbone_model.output_nc == 256


# ------------------------------------------------------------------------------------------------ the three quirks
class _Recorder(object):
    """the oracle kernels, with every furthest_point_sample call written down"""

    def __init__(self, oracle):
        self._o = oracle
        self.fps_calls = []

    def furthest_point_sample(self, xyz, n):
        self.fps_calls.append((xyz.detach().clone(), n))
        return self._o.furthest_point_sample(xyz, n)

    def __getattr__(self, k):
        return getattr(self._o, k)


def test_quirk_1_the_aggregation_samples_the_votes_and_only_once(oracle):
    g = vc.net_gold()
    rec = _Recorder(oracle)
    net = vc.build_net(g, CPU, kernels=rec, fused=False)
    votes = Data(pos=g["vote_pos"], x=g["vote_x"], seed_pos=g["down1_pos"], seed_inds=g["sampling_id_0"][:, :64])
    res = net.proposal_cls_module(votes)
    assert len(rec.fps_calls) == 1 and rec.fps_calls[0][1] == 16
    assert torch.equal(rec.fps_calls[0][0], g["vote_pos"])  # the votes, not seed_pos
    assert torch.equal(res.sampled_votes, g["sampled_votes"])
    idx = oracle.furthest_point_sample(g["vote_pos"], 16)
    assert torch.equal(idx, g["agg_idx"])
    assert not torch.equal(oracle.furthest_point_sample(g["down1_pos"], 16), idx), "the fixture does not tell the two apart"


def test_quirk_2_seed_indices_are_the_first_level_s(oracle):
    g = vc.net_gold()
    net = vc.build_net(g, CPU, kernels=oracle, fused=False)
    feats = net.backbone_model(Data(pos=g["pos"], x=g["x"]))
    seeds, inds = net._select_seeds(feats)
    assert torch.equal(inds, g["sampling_id_0"][:, :64]) and seeds.pos is feats.pos
    # They are first-level indices, not indices composed through the second level's own sampling.  With furthest point
    # sampling at both levels the two name the same points: sampling an FPS-ordered set again returns its prefix.
    assert torch.equal(oracle.furthest_point_sample(g["down0_pos"], 64), torch.arange(64).repeat(2, 1))
    assert torch.equal(g["pos"].gather(1, inds.unsqueeze(-1).expand(-1, -1, 3)), feats.pos)
    # the vote labels are gathered through them
    lab = vc.labels_of(g, CPU)
    res = V.VoteNetResults(seed_pos=feats.pos, seed_inds=inds, seed_votes=feats.pos + 0.1)
    want = (lab["vote_label"].gather(1, inds.unsqueeze(-1).expand(-1, -1, 9)).view(2, 64, 3, 3) - 0.1).abs().sum(-1).min(-1)[0]
    mask = lab["vote_label_mask"].gather(1, inds).float()
    torch.testing.assert_close(V.compute_vote_loss(lab, res), (want * mask).sum() / (mask.sum() + 1e-6))
    # a backbone without sampling ids: furthest point sampling of the feature positions, which also gathers
    net._num_seeds = 20
    bare = Data(pos=feats.pos, x=feats.x)
    seeds, inds = net._select_seeds(bare)
    assert torch.equal(inds, oracle.furthest_point_sample(feats.pos, 20)) and tuple(seeds.x.shape) == (2, 32, 20)
    assert torch.equal(seeds.pos, feats.pos.gather(1, inds.unsqueeze(-1).expand(-1, -1, 3)))


def test_quirk_3_tie_rules():
    vc.check_nms_tie_chain_and_degenerate(CPU)
    vc.check_matching_small_cases(CPU)


# ------------------------------------------------------------------------------------------------ the C-ABI
NEW_ENTRY_POINTS = ("tp3d_box_nms_f32", "tp3d_box3d_iou_f64", "tp3d_box_best_gt_f64", "tp3d_ap_match")


def test_detection_entry_points_header_binding_and_abi():
    from torch_points3d_amd import _lib, torchpoints
    text = open(os.path.join(ROOT, "include", "tp3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_ENTRY_POINTS:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert decl, name + " is not declared in include/tp3d_hip.h"
        assert len(_lib.SIGNATURES[name]) == decl.group(1).count(",") + 1, name
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+TP3D_ABI_VERSION\s+39\b", text) and _lib.ABI_VERSION == 39
    limit = int(re.search(r"#define\s+TP3D_BOX_NMS_MAX_BOXES\s+(\d+)", text).group(1))
    assert limit == torchpoints.BOX_NMS_MAX_BOXES == _lib.load().tp3d_box_nms_max_boxes() and limit >= 4096
    src = open(os.path.join(ROOT, "torch_points3d_amd", "csrc", "detection.hip")).read()
    assert "asm" not in src and "atomic" not in src.replace("no atomics", "")


def test_device_only_functions_refuse_cpu_tensors():
    from torch_points3d_amd import torchpoints as tp
    c = torch.zeros(1, 8, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.box3d_iou(c, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.box_nms(torch.zeros(1, 1, 6), torch.zeros(1, 1), torch.zeros(1, 1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.ap_match(c, torch.zeros(1), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), c,
                    torch.zeros(1, dtype=torch.int64), torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        V.box_nms(torch.zeros(1, 4097, 6), torch.zeros(1, 4097), torch.zeros(1, 4097, dtype=torch.int64))
    with pytest.raises(ValueError):
        tp.box_nms(torch.zeros(1, 4097, 6), torch.zeros(1, 4097), torch.zeros(1, 4097, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ boxes, numpy path
def test_known_answers_of_the_reference_s_box_tests():
    vc.check_corner_and_volume_known_answers(CPU)
    vc.check_intersection_area_known_answers(CPU)
    vc.check_nms_known_answers(CPU)
    vc.check_get_boxes_known_answer(CPU)
    vc.check_eval_detection_known_answer(CPU)


@pytest.mark.parametrize("B,P", vc.NMS_SHAPES)
def test_nms_fixture(B, P):
    vc.check_nms_fixture(CPU, B, P)


def test_iou_fixture():
    """the numpy path IS the restatement's arithmetic: bit-equal"""
    assert vc.check_iou_fixture(CPU, 0.0) == 0.0


def test_matching_fixture():
    vc.check_matching_fixture(CPU)


def test_get_boxes_fixture():
    vc.check_get_boxes_fixture(CPU)


def test_huber_and_nn_distance():
    from torch_points3d_amd.losses import huber_loss, nn_distance
    e = torch.tensor([-3.0, -1.0, -0.5, 0.0, 0.25, 1.0, 2.0])
    torch.testing.assert_close(huber_loss(e, 1.0), torch.tensor([2.5, 0.5, 0.125, 0.0, 0.03125, 0.5, 1.5]))
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(2, 5, 3, generator=g), torch.randn(2, 7, 3, generator=g)
    d = ((a[:, :, None] - b[:, None]) ** 2).sum(-1)
    d1, i1, d2, i2 = nn_distance(a, b)
    assert torch.equal(i1, d.argmin(2)) and torch.equal(i2, d.argmin(1))
    torch.testing.assert_close(d1, d.min(2)[0]) and torch.testing.assert_close(d2, d.min(1)[0])
    l1 = nn_distance(a, b, l1=True)[0]
    torch.testing.assert_close(l1, (a[:, :, None] - b[:, None]).abs().sum(-1).min(2)[0])


# ------------------------------------------------------------------------------------------------ the network, oracle kernels
def test_network_stages_on_the_fixture(oracle):
    g = vc.net_gold()
    vc.check_stages_teacher_forced(g, vc.build_net(g, CPU, kernels=oracle, fused=False), CPU)


def test_network_chained_pass_losses_gradients_and_eval(oracle):
    g = vc.net_gold()
    vc.check_chained_pass(g, vc.build_net(g, CPU, kernels=oracle, fused=False), CPU)


def test_losses_take_a_dict_or_an_object():
    g = vc.net_gold()
    res = V.VoteNetResults.from_logits(
        g["sampling_id_0"][:, :64], g["vote_pos"], g["down1_pos"], g["sampled_votes"],
        torch.cat([g[k].reshape(2, 16, -1) for k in ("objectness_scores",)] + [g["center"] - g["sampled_votes"]] + [
            g[k].reshape(2, 16, -1) for k in ("heading_scores", "heading_residuals_normalized", "size_scores",
                                              "size_residuals_normalized", "sem_cls_scores")], -1).transpose(1, 2),
        4, 1, torch.tensor(vc.MEAN_SIZE))
    params = dict(objectness_cls_weights=[0.2, 0.8], num_heading_bin=1, mean_size_arr=vc.MEAN_SIZE)
    out = []
    for make in (dict, lambda d: Data(**d)):
        lab = make({k: v.clone() for k, v in vc.labels_of(g, CPU).items()})
        res.assign_objects(g["label/center_label"], g["label/box_label_mask"], 0.3, 0.6)
        out.append(V.get_loss(lab, res, params))
    for k in vc.LOSS_KEYS:
        assert float(out[0][k]) == float(out[1][k])
        assert abs(float(out[0][k]) - float(g["f64/loss/" + k])) <= max(1e-5, 4 * abs(float(g["loss/" + k]) - float(g["f64/loss/" + k])))
