"""Host-side plans of the few-row tile rule (csrc/gemm_plans.h; no GPU): the 64 x 64 form of the plain rows GEMM
(tp3d_gemm_rows_small_plan) and the tile choice of the fp32 weight-gradient GEMM (tp3d_gemm_tn_plan), under both settings
of fused.FEW_ROW_TILES, over the ROWS x CHANNELS grid of test_plans_cpu.py (the two lists are copies).  Also builds and
runs the stand-alone sweep tests/guard/few_row_plans_main.cpp under the host sanitizers."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from torch_points3d_amd import _lib, fused

ROWS = sorted(set(
    [1, 2, 3, 31, 32, 33, 63, 64, 65, 120, 127, 128, 129, 255, 256, 257, 480, 512, 1000, 1023, 1024, 1025, 2048, 2100,
     3840, 4095, 4096, 4097, 8191, 8192, 11520, 16384, 65535, 65536, 65537, 130047, 130048, 130049, 130176, 130177,
     130944, 131071, 131072, 131073, 262144, 524288, 1048575, 1048576, 1048577, 2097152, 4194304]
    + [128 * k + d for k in (1016, 1017, 1020, 1023, 1024, 1025) for d in (-1, 0, 1)]))
CHANNELS = [1, 3, 4, 6, 8, 10, 13, 16, 20, 24, 32, 48, 50, 64, 96, 128, 131, 132, 192, 196, 256, 259, 260, 320, 323, 384,
            512, 515, 516, 1024, 1280, 1536]


def _plan(name, n, *args):
    buf = (ctypes.c_int64 * n)()
    rc = getattr(_lib.load(), name)(*args, ctypes.addressof(buf))
    assert rc == 0, (name, args, rc)
    return list(buf)


@pytest.fixture
def few_row():
    """few_row(v): route the library by fused.FEW_ROW_TILES = v; the default is put back afterwards"""
    saved = fused.FEW_ROW_TILES

    def use(v):
        fused.FEW_ROW_TILES = v
        fused.sync_few_row_tiles()
    yield use
    use(saved)


def test_rows_small_plan_routes_only_few_wide_unsplit_items(few_row):
    h = _lib.load()
    routed = 0
    for M in ROWS:
        for N, K in itertools.product(CHANNELS, [0, 4, 256, 260, 512, 1024, 1280, 1536]):
            few_row(0)
            assert _plan("tp3d_gemm_rows_small_plan", 4, M, N, K) == [0, 0, 0, 0], (M, N, K)
            old = _plan("tp3d_gemm_rows_plan", 9, M, N, K)
            chunks0, floats0 = h.tp3d_gemm_rows_stat_chunks(M, N), h.tp3d_gemm_rows_stat_floats(M, N)
            few_row(1)
            assert _plan("tp3d_gemm_rows_plan", 9, M, N, K) == old, (M, N, K)  # the nine fields keep their meaning
            assert (chunks0, floats0) == (h.tp3d_gemm_rows_stat_chunks(M, N), h.tp3d_gemm_rows_stat_floats(M, N)), (M, N)
            items, wgs, with_stats, without = _plan("tp3d_gemm_rows_small_plan", 4, M, N, K)
            tiles_n, row_blocks, items128, _, chunks, per_wg, wave_rows, ksplit, bn = old
            few = bn == 128 and items128 <= 256
            assert with_stats == int(few), (M, N, K)          # a launch with statistics is never K-split
            assert without == int(few and ksplit == 1), (M, N, K)
            if with_stats:
                routed += 1
                assert items == wgs == 4 * items128 <= 1024, (M, N, K)
                assert not per_wg and chunks == 2 * row_blocks  # one chunk per (128-row block, 64-row half), as before
            else:
                assert (items, wgs, without) == (0, 0, 0), (M, N, K)
    assert routed > 1000
    for M, N, K in ((4096, 256, 260), (4096, 256, 256), (4096, 512, 256), (16384, 128, 256)):  # the step's under-filled layers
        assert _plan("tp3d_gemm_rows_small_plan", 4, M, N, K)[2:] == [1, 1], (M, N, K)
    assert _plan("tp3d_gemm_rows_small_plan", 4, 4096, 256, 1280)[2:] == [1, 0]  # the K-split decoder layer keeps its route


def _tn_reference(M, N, K):
    """plan_tn's formula for the row split, from M, N, K alone: (tile rows, tile columns, gn == 1 form, splits, rows per split)"""
    wm = 2 if N > 64 else 1
    if K <= 64:
        wn = 1
    elif K <= 128:
        wn = 2
    elif K <= 192:
        wn = 3
    else:
        wn = 3 if -(-K // 192) * 192 < -(-K // 128) * 128 else 2
    gn = 2
    if N <= 32 and K >= 128:
        gn, wm, wn = 1, 1, 1
    tn, tk = 32 * gn * wm, 32 * (4 // gn) * wn
    tiles = -(-N // tn) * -(-K // tk)
    want = -(-1024 // tiles)
    s = max(1, min(want, -(-M // 256), 512))
    rps = -(-(-(-M // s)) // 64) * 64
    return tn, tk, gn == 1, wn == 3, tiles, -(-M // rps), rps


def test_gemm_tn_tile_follows_the_fill_and_leaves_the_row_split(few_row):
    changed = 0
    for M in ROWS:
        for N, K in itertools.product(CHANNELS, CHANNELS):
            if N * K > 1024 * 1280:
                continue
            tn0, tk0, one_row, wide3, tiles0, splits, rps = _tn_reference(M, N, K)
            few_row(0)
            old = _plan("tp3d_gemm_tn_plan", 8, M, N, K)
            assert old[:5] == [splits, rps, tn0, tk0, tiles0], (M, N, K)
            few_row(1)
            new = _plan("tp3d_gemm_tn_plan", 8, M, N, K)
            assert new[:2] == [splits, rps] and new[6:] == old[6:], (M, N, K)  # summation order and workspace extent
            tn, tk, tiles, staged = new[2:6]
            assert tiles * tn * tk >= N * K and rps % staged == 0, (M, N, K)
            if one_row or wide3 or tiles0 * splits >= 256:
                assert new == old, (M, N, K)
                continue
            assert (tn, tk) in ((128, 128), (128, 64), (64, 128), (64, 64)) and tn <= tn0 and tk <= tk0, (M, N, K)
            assert tiles * splits >= tiles0 * splits
            if (tn, tk) != (64, 64) and (tn, tk) != (tn0, tk0):
                assert tiles * splits >= 256, (M, N, K)  # a half-size tile only where it fills the CUs
            changed += (tn, tk) != (tn0, tk0)
    assert changed > 100
    few_row(1)
    for (M, N, K), tile in (((4096, 256, 256), (64, 64)), ((4096, 256, 260), (64, 64)), ((4096, 512, 256), (128, 64)),
                            ((16384, 128, 256), (128, 64))):
        assert tuple(_plan("tp3d_gemm_tn_plan", 8, M, N, K)[2:4]) == tile, (M, N, K)


def test_plan_sweep_under_the_host_sanitizers(tmp_path):
    """tests/guard/few_row_plans_main.cpp: the planning header compiled without a device, as a program of its own, run on
    the CPU -- with AddressSanitizer and UBSan on a machine without a GPU (sanitizers stay off the GPU machines; there,
    and where the compiler has no sanitizer runtime, the plain build runs the same checks)"""
    import torch
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "few_row_plans")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "torch_points3d_amd", "csrc"),
            os.path.join(ROOT, "tests", "guard", "few_row_plans_main.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if torch.cuda.is_available() or subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.check_call(base)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
