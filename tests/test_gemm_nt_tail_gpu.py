"""GPU: the four-wave NT kernel's one launch on all rows (256-row tiles, then 128-row tiles that fill the last round) against the 8-wave
kernel alone (VITK_NT_W128=0), bit for bit.

Both kernels form every output element from the same MFMA products in the same K order, so C, aux and the 8-bit gelu' codes must be
identical whatever the row split.  Cells: the ViT-B/16 batch-256 shapes (M = 50,432), ViT-L/16 at batch 128 (M = 25,216), an M that is an
odd number of 128-row tiles (M % 256 == 128), an M one 128-row tile above a whole round, and an M % 128 != 0 (the two-launch split);
each under CU reserve 0, 32 and 192 (the launch grid follows the reserve).  Outputs sit between guard rows; everything is NaN-filled
before the call.  Afterwards every output element must be finite and every guard row unchanged, and a second run must be bit-identical."""
import os

import pytest
import torch

from vit_pytorch_amd import _lib as L
from vit_pytorch_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 8           # guard rows above and below every output
BF = torch.bfloat16

E = {"none": L.EPI_NONE, "bias": L.EPI_BIAS, "bias_gelu": L.EPI_BIAS_GELU, "resid": L.EPI_RESID, "resid16": L.EPI_RESID16,
     "dg": L.EPI_BIAS_GELU_DG, "dg8": L.EPI_BIAS_GELU_DG8}
ALL = list(E)
SHAPES = [
    (50432, 768, 3072, ALL),                              # FF2 / dX of FF1: 2.31 rounds at N = 768
    (50432, 768, 768, ["none", "resid", "resid16"]),     # out-projection, dX of the out-projection
    (50432, 768, 2304, ["none"]),                         # dX of QKV
    (50432, 3072, 768, ["none", "bias_gelu", "dg", "dg8"]),   # FF1 (9.23 rounds)
    (50432, 2304, 768, ["bias"]),                         # QKV
    (25216, 1024, 4096, ["none", "resid16"]),            # ViT-L/16 batch 128
    (25216, 4096, 1024, ["dg8"]),
    (3200, 768, 768, ALL),                                # 25 128-row tiles: M % 256 == 128
    (22144, 768, 768, ["none", "resid16", "dg8"]),       # 86.5 m-tiles: one 128-row tile past a whole round on 256 CUs
    (5000, 768, 3072, ["none", "resid"]),                 # M % 128 != 0: the two-launch split
]
RESERVES = [0, 32, 192]


@pytest.fixture(autouse=True)
def _clean():
    os.environ.pop("VITK_NT_W128", None)
    yield
    os.environ.pop("VITK_NT_W128", None)
    K.set_cu_reserve(0)


def guarded(M, N, dtype, fill):
    buf = torch.empty((M + 2 * G, N), dtype=dtype, device=DEV)
    buf.fill_(fill)
    return buf


def run(A, W, bias, r32, r16, M, N, Kd, epi):
    e = E[epi]
    f32 = epi == "resid"
    C = guarded(M, N, torch.float32 if f32 else BF, float("nan"))
    aux = None
    if epi in ("bias_gelu", "dg"):
        aux = guarded(M, N, BF, float("nan"))
    elif epi == "dg8":
        aux = guarded(M, N, torch.uint8, 0xA5)
    resid = r32 if epi == "resid" else (r16 if epi == "resid16" else None)
    K.gemm_nt_bf16(A, Kd, W, Kd, C[G:G + M], N, M, N, Kd, e, bias=None if epi == "none" else bias, resid=resid,
                   aux=None if aux is None else aux[G:G + M])
    torch.cuda.synchronize()
    return C, aux


def same(x, y):
    return torch.equal(x.view(torch.uint8) if x.dtype != torch.uint8 else x, y.view(torch.uint8) if y.dtype != torch.uint8 else y)


@pytest.mark.parametrize("M,N,Kd,epis", SHAPES, ids=[f"M{m}_N{n}_K{k}" for m, n, k, _ in SHAPES])
def test_one_launch_matches_the_8wave_kernel_bit_for_bit(M, N, Kd, epis):
    g = torch.Generator(device=DEV)
    g.manual_seed(M + 7 * N + 13 * Kd)
    A = (torch.randn(M, Kd, generator=g, device=DEV)).to(BF)
    W = (torch.randn(N, Kd, generator=g, device=DEV) * 0.05).to(BF)
    bias = (torch.randn(N, generator=g, device=DEV) * 0.5).to(BF)
    r32 = torch.randn(M, N, generator=g, device=DEV)
    r16 = torch.randn(M, N, generator=g, device=DEV).to(BF)
    for epi in epis:
        os.environ["VITK_NT_W128"] = "0"
        C0, X0 = run(A, W, bias, r32, r16, M, N, Kd, epi)
        os.environ.pop("VITK_NT_W128")
        assert torch.isfinite(C0[G:G + M].float()).all(), (epi, "8-wave reference")
        for c in RESERVES:
            K.set_cu_reserve(c)
            outs = [run(A, W, bias, r32, r16, M, N, Kd, epi) for _ in range(2)]
            K.set_cu_reserve(0)
            tag = (M, N, Kd, epi, f"reserve {c}")
            for C, X in outs:
                assert torch.isnan(C[:G]).all() and torch.isnan(C[G + M:]).all(), (tag, "C guard rows written")
                assert torch.isfinite(C[G:G + M].float()).all(), (tag, "C rows not written")
                bad = (C[G:G + M].view(torch.int16 if C.dtype == BF else torch.int32) != C0[G:G + M].view(torch.int16 if C.dtype == BF else torch.int32))
                assert not bad.any(), (tag, "C differs from VITK_NT_W128=0", int(bad.sum()), bad.nonzero()[:4].tolist())
                if X is not None:
                    if X.dtype == torch.uint8:
                        assert (X[:G] == 0xA5).all() and (X[G + M:] == 0xA5).all(), (tag, "aux guard rows written")
                    else:
                        assert torch.isnan(X[:G]).all() and torch.isnan(X[G + M:]).all(), (tag, "aux guard rows written")
                        assert torch.isfinite(X[G:G + M].float()).all(), (tag, "aux rows not written")
                    assert same(X, X0), (tag, "aux differs from VITK_NT_W128=0")
            assert same(outs[0][0], outs[1][0]), (tag, "second run differs")
            if outs[0][1] is not None:
                assert same(outs[0][1], outs[1][1]), (tag, "second run differs (aux)")


def test_headline_shape_runs_as_one_launch():
    """With the plan in use, the N = 768 shapes at M = 50,432 take 128-row tiles (the plan query says so for the full chip)."""
    import ctypes
    lib = L.load()
    out = (ctypes.c_int32 * 4)()
    g = K.gemm_nt_plan(50432, 768, 3072, 768)["workgroups"]
    assert lib.vitk_gemm_nt_w128_plan(50432, 768, 3072, g, ctypes.cast(out, ctypes.c_void_p)) == 0
    assert 256 * out[0] + 128 * out[1] == 50432
    if g == 256:
        assert out[1] > 0
