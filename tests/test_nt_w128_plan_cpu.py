"""CPU: the one-launch plan of the four-wave NT kernel (gemm_ntw_plan, queried through vitk_gemm_nt_w128_plan; nothing is launched).

Where M % 128 == 0 and the epilogue has no column sums, the four-wave kernel takes all M rows in one launch: 256-row tiles, then
128-row tiles that fill the last round.  The plan must cover every row exactly once, and its modelled makespan must be no worse than
the two-launch split it replaces (the four-wave launch on gemm_ntw_split's rows, then the 8-wave launch on the rest)."""
import ctypes

import pytest

from vit_pytorch_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def plan(lib, M, N, K, grid):
    out = (ctypes.c_int32 * 4)()
    assert lib.vitk_gemm_nt_w128_plan(M, N, K, grid, ctypes.cast(out, ctypes.c_void_p)) == 0
    return list(out)


# ViT-B/16 at batch 256 (M = 50,432) and ViT-L/16 at batch 128 (M = 25,216): every NT GEMM of the step
VIT_B = [(50432, n, k) for n, k in ((2304, 768), (768, 768), (3072, 768), (768, 3072), (768, 2304))]
VIT_L = [(25216, n, k) for n, k in ((3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (1024, 3072))]
GRIDS = [256, 224, 64]      # reserve 0, 32, 192


@pytest.mark.parametrize("M,N,K", VIT_B + VIT_L + [(3200, 768, 768), (22144, 768, 768), (384, 256, 256)])
@pytest.mark.parametrize("grid", GRIDS)
def test_plan_covers_every_row_and_is_no_worse_than_the_split(lib, M, N, K, grid):
    tm, th, cost, split_cost = plan(lib, M, N, K, grid)
    assert tm >= 0 and th >= 0 and 256 * tm + 128 * th == M, (M, N, K, grid, tm, th)
    assert 0 < cost <= split_cost, (M, N, K, grid, cost, split_cost)
    # never more than one round of 256-row tiles re-cut: the 128-row tiles only fill the last round
    assert th * (N // 256) <= 2 * (grid + N // 256), (M, N, K, grid, th)


def test_partial_last_round_is_filled_at_the_headline(lib):
    """ViT-B/16 N = 768 (FF2, the out-projection and the dX of FF1 / QKV): 591 tiles = 2.31 rounds on 256 workgroups; the one-launch
    plan models about 2.55 rounds where a single launch of 256-row tiles takes 3."""
    for K in (768, 2304, 3072):
        tm, th, cost, split_cost = plan(lib, 50432, 768, K, 256)
        assert th > 0 and cost < 2700 and cost < split_cost, (K, tm, th, cost, split_cost)


@pytest.mark.parametrize("M,N,K", [(50433, 768, 768), (5000, 768, 3072), (50432, 768, 224), (50432, 200, 768), (128, 768, 768)])
def test_shapes_outside_the_one_launch_plan(lib, M, N, K):
    """M % 128 != 0 and shapes gemm_ntw_serves refuses keep the two-launch route: the query reports zeros."""
    assert plan(lib, M, N, K, 256) == [0, 0, 0, 0]


def test_grid_is_checked(lib):
    out = (ctypes.c_int32 * 4)()
    assert lib.vitk_gemm_nt_w128_plan(50432, 768, 768, 12, ctypes.cast(out, ctypes.c_void_p)) != 0
    assert lib.vitk_gemm_nt_w128_plan(50432, 768, 768, 0, ctypes.cast(out, ctypes.c_void_p)) != 0
