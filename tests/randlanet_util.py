"""Shared by tests/test_randlanet_cpu.py and tests/test_gpu_randlanet.py: the fixtures of
tests/golden/make_golden_randlanet.py (the reference's RandLA-Net segmentation networks), this package's RandLANetSeg
on their weights, their recorded draws replayed, and the float64 statement of the eval-mode edge pass."""
import torch

from conftest import load_golden
from randla_golden_util import Replay

FEAT, CLASSES = 3, 5
CONFIGS = ("Randlanet_Conv", "Randlanet_Res")


def load_fixture(name):
    """one config's arrays; Randlanet_Res is split over two archives (1 MiB per committed file)"""
    if name == "Randlanet_Conv":
        return load_golden("randlanet")
    gold = load_golden("randlanet_res")
    gold.update(load_golden("randlanet_res_grads"))
    return gold


def state_of(gold):
    return {k[len("sd/"):]: v for k, v in gold.items() if k.startswith("sd/")}


def draws_of(gold):
    return [gold["draw%d" % i] for i in range(int(gold["ndraws"][0]))]


def samplers(net):
    """every RandlaConv of the network, in the order their samplers draw in a forward"""
    from torch_points3d_amd.randla import RandlaConv
    return [m for m in net.modules() if isinstance(m, RandlaConv)]


def build_net(name, gold, device, lfa, dtype=torch.float32):
    """RandLANetSeg on the fixture's weights (strict load: the reference's keys, all of them); no dropout, as in the
    generator's head"""
    from torch_points3d_amd.randla import RandLANetSeg
    net = RandLANetSeg(name, FEAT, CLASSES, lfa=lfa)
    net.load_state_dict(state_of(gold), strict=True)
    net.dropout = 0.0
    return net.to(device=device, dtype=dtype)


def replay(net, draws, device, sort=False):
    """the samplers of `net` hand out `draws` in turn (sorted first with sort=True, as RandomSampler(sort=True) does)"""
    if sort:
        draws = [torch.sort(d)[0] for d in draws]
    r = Replay(draws, device)
    convs = samplers(net)
    assert len(convs) == len(draws), (len(convs), len(draws))
    for conv in convs:
        conv.sampler = r
    return r


def bag(gold, device, dtype=torch.float32, x=None):
    from torch_points3d_amd.kpconv_blocks import PDData
    x = gold["x"] if x is None else x
    return PDData(pos=gold["pos"].to(device=device, dtype=dtype), batch=gold["batch"].to(device),
                  x=x.to(device=device, dtype=dtype))


def lfa_fp64(pos_q, pos_s, x, nbr, point_pos_nn, attention_nn):
    """RandlaKernel's rows arithmetic up to the sum over the neighbours (randla.py RandlaKernel.forward, CPU branch),
    eval mode, evaluated in double on the CPU: the float64 side of the kernel tests.  The MLPs are deep-copied to double."""
    import copy
    import torch.nn.functional as F
    pp = copy.deepcopy(point_pos_nn).cpu().double().eval()
    at = copy.deepcopy(attention_nn).cpu().double().eval()
    pos_q, pos_s, nbr = pos_q.cpu().double(), pos_s.cpu().double(), nbr.cpu()
    Nq, k = nbr.shape
    j = nbr.reshape(-1)
    pos_i = pos_q.repeat_interleave(k, dim=0)
    pos_j = pos_s[j]
    x_j = pos_j if x is None else x.cpu().double()[j]
    vij = pos_i - pos_j
    dij = torch.norm(vij, dim=1).unsqueeze(1)
    with torch.no_grad():
        rij = pp(torch.cat([pos_i, pos_j, vij, dij], dim=1))
        fij_hat = torch.cat([x_j, rij], dim=1)
        msg = F.softmax(at(fij_hat), -1) * fij_hat
    return msg.reshape(Nq, k, -1).sum(dim=1)
