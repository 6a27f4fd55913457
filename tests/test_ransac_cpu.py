"""RANSAC registration without a GPU: ransac_registration's numpy path on the reference's own test_ransac
(test/test_registration_metrics.py:61-72, rtol 1e-3) and against the float64 restatement of
tests/registration_ransac_ref.py for given samples; compute_metrics' keys; the new header entries through cabi."""
import ctypes
import os
import shutil
import subprocess

import numpy.testing as npt
import pytest
import torch

import registration_ransac_ref as ref
import registration_ref as rr
from conftest import ROOT

FGR_KEYS = ["trans_error_fgr", "rot_error_fgr", "rre_fgr", "rte_fgr", "sr_fgr"]


@pytest.fixture(scope="module")
def reg():
    from torch_points3d_amd import registration
    return registration


def test_case_a_pose_has_no_small_entry():
    """assert_allclose(T, T_gt, rtol=1e-3) has no absolute term: it only means something where no entry is near 0"""
    _, _, T = ref.case_a()
    assert float(T[:3].abs().min()) >= 0.05
    assert abs(float(torch.det(T[:3, :3].double())) - 1) < 1e-6


def test_ransac_registration_reproduces_the_reference_test(reg):
    a, b, T_gt = ref.case_a()
    gen = torch.Generator().manual_seed(7)
    T = reg.ransac_registration(a, b, distance_threshold=0.01, num_iterations=4096, generator=gen)
    assert T.dtype == torch.float32 and T.shape == (4, 4) and T.device.type == "cpu"
    npt.assert_allclose(T.numpy(), T_gt.numpy(), rtol=1e-3)
    again = reg.ransac_registration(a, b, distance_threshold=0.01, num_iterations=4096, generator=gen.manual_seed(7))
    assert torch.equal(T, again)


@pytest.mark.parametrize("case,threshold,n", [("a", 0.01, 4), ("b", 0.05, 4), ("b", 0.05, 3)])
def test_numpy_path_matches_the_restatement(reg, case, threshold, n):
    xyz, tgt, _ = ref.case_a() if case == "a" else ref.case_b(257, 257)
    samples = ref.draw(len(xyz), 513, n, 3)
    pose, best, counts = reg._ransac_numpy(xyz.numpy(), tgt.numpy(), threshold, samples.numpy())
    poses64 = ref.hypotheses(xyz, tgt, samples)
    lo, mid, hi = ref.counts_banded(poses64, xyz, tgt, threshold, 1e-9)
    counts = torch.from_numpy(counts)
    keep = ref.well_posed(xyz, tgt, samples)  # (elsewhere Horn and the SVD may take different poses of equal residual)
    print("ill-posed hypotheses: %d of %d" % (int((~keep).sum()), len(keep)))
    assert float((~keep).double().mean()) <= ref.ill_posed_allowance(len(xyz), n)
    assert bool((lo <= counts)[keep].all()) and bool((counts <= hi)[keep].all()) and float((hi - lo).double().mean()) < 1e-2
    assert best == int(torch.nonzero(counts == counts.max())[0])  # the first of the best
    if case == "a":
        assert int(counts.max()) == 90 and int((counts == 90).sum()) > 100  # (the lowest-index rule has ties to break)
    horn = torch.from_numpy(reg._horn_numpy(xyz.double().numpy()[samples.numpy()], tgt.double().numpy()[samples.numpy()]))
    scale = 1.0 + poses64[keep].abs()
    assert float(((horn[keep] - poses64[keep]).abs() / scale).max()) < 1e-9  # Horn and SVD-Kabsch: the same pose
    want, inliers, _, margin = ref.refit(xyz, tgt, threshold, poses64[best])
    assert margin > 1e-7 and inliers >= (90 if case == "a" else 150)
    npt.assert_allclose(pose, want.numpy(), rtol=1e-9, atol=1e-11)
    T = reg.ransac_registration(xyz, tgt, threshold, samples=samples)
    npt.assert_allclose(T[:3].numpy(), want.float().numpy(), rtol=1e-6, atol=1e-7)


def test_numpy_path_edges(reg):
    gen = torch.Generator().manual_seed(0)
    xyz, tgt = torch.rand(50, 3, generator=gen), torch.rand(50, 3, generator=gen) * 7
    samples = ref.draw(50, 64, 4, 1)
    T = reg.ransac_registration(xyz, tgt, 1e-3, samples=samples)  # all outliers: the hypothesis' own pose, finite
    pose, best, counts = reg._ransac_numpy(xyz.numpy(), tgt.numpy(), 1e-3, samples.numpy())
    assert counts.max() < 3 and bool(torch.isfinite(T).all())
    npt.assert_allclose(T[:3].numpy(), ref.hypotheses(xyz, tgt, samples)[best].float().numpy(), rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        reg.ransac_registration(xyz[:2], tgt[:2])
    with pytest.raises(ValueError):
        reg.ransac_registration(xyz, tgt, num_iterations=0)
    with pytest.raises(ValueError):
        reg.ransac_registration(xyz, tgt, samples=samples[:, :2])


def test_torchpoints_operators_check_their_arguments():
    from torch_points3d_amd import torchpoints as tp
    xyz, samples = torch.rand(10, 3), torch.zeros(4, 4, dtype=torch.long)
    for call in (lambda: tp.ransac_score(xyz, xyz, samples, 0.1), lambda: tp.kabsch(xyz, xyz),
                 lambda: tp.ransac_pose(xyz, xyz, 0.1, samples=samples)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # (the refusal every other operator gives)
            call()
    assert tp.RANSAC_TILE >= 64 and tp.RANSAC_HYP_BLOCK >= 64


def test_compute_metrics_keys(reg, monkeypatch):
    """the script's keys without its time_* entries; get_matches and FGR are device-only, so their CPU restatements stand in"""
    monkeypatch.setattr(reg, "get_matches", rr.get_matches)
    monkeypatch.setattr(reg, "fast_global_registration", rr.fast_global_registration)
    xyz, tgt, T = ref.case_b(200, 5)
    gen = torch.Generator().manual_seed(2)
    feat = torch.randn(200, 16, generator=gen)
    feat = feat / feat.norm(dim=1, keepdim=True)
    feat_t = feat + 0.01 * torch.randn(200, 16, generator=gen)
    T = T.float()
    base = ["hit_ratio", "feat_match_ratio"] + FGR_KEYS
    res = reg.compute_metrics(xyz, tgt, feat, feat_t, T)
    assert sorted(res) == sorted(base) and all(torch.is_tensor(v) and v.dim() == 0 for v in res.values())
    res = reg.compute_metrics(xyz, tgt, feat, feat_t, T, xyz_gt=xyz, xyz_target_gt=tgt)
    assert sorted(res) == sorted(base + ["registration_recall_fgr"])
    res = reg.compute_metrics(xyz, tgt, feat, feat_t, T, use_ransac=True, ransac_thresh=0.05, xyz_gt=xyz, xyz_target_gt=tgt,
                              ransac_iterations=512, generator=gen)
    ransac = [k.replace("fgr", "ransac") for k in FGR_KEYS + ["registration_recall_fgr"]]
    assert sorted(res) == sorted(base + ["registration_recall_fgr"] + ransac)
    assert float(res["rre_ransac"]) == 1.0 and float(res["rte_ransac"]) == 1.0 and float(res["trans_error_ransac"]) < 0.01
    with pytest.raises(TypeError):
        reg.compute_metrics(xyz, tgt, feat, feat_t, T, use_teaser=True)


def test_header_entries_parse(reg):
    from torch_points3d_amd import _lib, cabi
    functions, constants = cabi.parse_header(os.path.join(ROOT, "include", "tp3d_hip.h"))
    i, l, f, d, z, p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p
    want = {"tp3d_ransac_workspace_bytes": (z, [l, l]),
            "tp3d_ransac_splits": (i, [l, l]),
            "tp3d_ransac_score_f32": (i, [p, p, l, p, l, i, f, p, p, p, z, p]),
            "tp3d_ransac_select": (i, [p, p, l, p, l, i, p, p, z, p]),
            "tp3d_kabsch_accumulate_f32": (i, [p, p, p, l, i, d, p, z, p]),
            "tp3d_kabsch_solve": (i, [l, i, i, p, p, z, p])}
    for name, (restype, argtypes) in want.items():
        assert functions[name][0] is restype and functions[name][1] == argtypes, name
        assert _lib.FUNCTIONS[name] == functions[name]
    assert constants["TP3D_RANSAC_TILE"] == 256 and constants["TP3D_RANSAC_HYP_BLOCK"] == 256
    from torch_points3d_amd import torchpoints as tp
    assert tp.RANSAC_TILE == constants["TP3D_RANSAC_TILE"] and tp.RANSAC_HYP_BLOCK == constants["TP3D_RANSAC_HYP_BLOCK"]
    doc = reg.__doc__
    assert "RANSAC (open3d)" not in doc and "ransac_registration" in doc


def test_horn_header_under_the_host_sanitizers(tmp_path):
    """tests/guard/ransac_horn_main.cpp: csrc/ransac_horn.h, the text the kernels compile, as a host program of its own --
    with AddressSanitizer and UBSan on a machine without a GPU (sanitizers stay off the GPU machines; there, and where
    the compiler has no sanitizer runtime, the plain build runs the same checks)"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ransac_horn")
    base = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + os.path.join(ROOT, "torch_points3d_amd", "csrc"),
            os.path.join(ROOT, "tests", "guard", "ransac_horn_main.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if torch.cuda.is_available() or subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.check_call(base)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
