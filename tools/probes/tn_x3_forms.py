"""Device time of every form of the bf16-pipe weight-gradient kernel (csrc/gemm_tn_x3.hip) at the training step's shapes:
plain rows, activated operand formed by the loaders, and the same with the reductions of the layer below, each with the
1, 6 and 9 term-pair MFMA work where the entry point takes it.  HIP events, best of five rounds.

    python tools/probes/tn_x3_forms.py [reps] [out.json]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from torch_points3d_amd import _lib, fused  # noqa: E402

DEV = "cuda:0"
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else None


def timeit(fn):
    for _ in range(3):
        fn()
    best = float("inf")
    for _ in range(5):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / reps * 1e3)
    return best


rows = []
h = _lib.load()
for M, N, K in [(524288, 128, 128), (1048576, 128, 64), (1048576, 64, 64), (262144, 256, 128), (524288, 128, 132)]:
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    dY = torch.randn(M, N, generator=g, device=DEV)
    Yp = torch.randn(M, K, generator=g, device=DEV) * 1.5 + 0.2
    dA = torch.randn(M, K, generator=g, device=DEV)
    mean, invstd = Yp.mean(0), 1.0 / torch.sqrt(Yp.var(0, unbiased=False) + 1e-5)
    scale, beta = (torch.rand(K, generator=g, device=DEV) + 0.5) * invstd, torch.randn(K, generator=g, device=DEV) * 0.3
    act = (mean, scale, beta, 0.01)
    st = _lib.stream_ptr(dY.device)
    row = {"M": M, "N": N, "K": K}
    for rev in (0, 1):
        sfx = "_rev" if rev else ""
        row["one_pair_us" + sfx] = timeit(lambda: fused.gemm_tn(dY, Yp, x3=1, reverse=rev))
        row["six_pairs_us" + sfx] = timeit(lambda: fused.gemm_tn(dY, Yp, x3=6, reverse=rev))
        row["nine_pairs_us" + sfx] = timeit(lambda: fused.gemm_tn(dY, Yp, x3=9, reverse=rev))
        row["six_pairs_act_us" + sfx] = timeit(lambda: fused.gemm_tn(dY, Yp, x3=6, act=act, reverse=rev))
        chunks = h.tp3d_gemm_tn_x3_red_chunks(M, N, K)
        if chunks:
            ws = _lib.gemm_tn_workspace(M, N, K, dY.device, x3=True)
            rws = torch.empty(chunks * 2 * K, device=DEV)
            out, red = torch.empty(N, K, device=DEV), torch.empty(4, K, device=DEV)
            row["six_pairs_act_red_us" + sfx] = timeit(lambda: _lib.call(
                "tp3d_gemm_tn_x3_act_red_f32", _lib.ptr(dY), _lib.ptr(Yp), _lib.ptr(mean), _lib.ptr(scale), _lib.ptr(beta),
                _lib.ptr(invstd), 0.01, _lib.ptr(dA), 1, M, N, K, 6, _lib.ptr(out), _lib.ptr(ws), _lib.ptr(red), _lib.ptr(rws), rev, st))
            row["act_red_TBps" + sfx] = 4.0 * M * (N + 2 * K) / row["six_pairs_act_red_us" + sfx] / 1e6
    rows.append(row)
    print(json.dumps({k: (round(v, 1) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
