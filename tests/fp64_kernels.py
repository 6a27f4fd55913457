"""A kernels namespace (what dense.py reads through `kernels=`) that evaluates the reference graph in the dtype of the
features: PointNet2Unet(..., kernels=fp64_kernels, fused=False) on double weights and features is a float64 evaluation of
the network, the counterpart of tests/golden/make_golden.py's _Fp64Kernels for tests that build their reference on the
fly (test_gpu_headline_fp64.py).

Indices (furthest point sampling, ball query, 3-NN) come from the CPU oracle on the fp32 coordinates, so every evaluation
shares the geometry of the fp32 passes; distances, gathers and interpolation are computed in the features' dtype."""
import torch

from oracle import tpk_ref

MAX_THREADS = 16


def limit_threads(n=MAX_THREADS):
    """at most n threads for torch and the oracle (never sized by the machine's core count)"""
    n = max(1, min(int(n), MAX_THREADS))
    torch.set_num_threads(min(torch.get_num_threads(), n))
    tpk_ref.set_num_threads(min(tpk_ref.num_threads(), n))


def furthest_point_sample(xyz, npoint):
    return tpk_ref.furthest_point_sample(xyz.float(), npoint)


def ball_query(radius, nsample, x, y, **kw):
    return tpk_ref.ball_query(radius, nsample, x.float(), y.float(), **kw)


def grouping_operation(features, idx):
    """out[b, c, j, s] = features[b, c, idx[b, j, s]] in the features' dtype (differentiable through gather)"""
    B, C, _ = features.shape
    return features.gather(2, idx.reshape(B, 1, -1).expand(B, C, -1)).reshape(B, C, *idx.shape[1:])


def three_nn(unknown, known):
    """the oracle's 3-NN indices on the fp32 coordinates; their distances in the coordinates' dtype"""
    _, idx = tpk_ref.three_nn(unknown.float(), known.float())
    B, n, _ = idx.shape
    nb = known.gather(1, idx.reshape(B, -1, 1).expand(B, n * 3, 3)).reshape(B, n, 3, 3)
    return ((nb - unknown.unsqueeze(2)) ** 2).sum(-1).sqrt(), idx


def three_interpolate(features, idx, weight):
    return (grouping_operation(features, idx) * weight.unsqueeze(1)).sum(-1)
