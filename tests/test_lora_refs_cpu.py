"""The fp64 reference of the LoRA products (tests/ref_lora.py) proven against an independent einsum formulation that gathers w(c, j)
element by element, and the torch stand-ins (tests/standin_lora.py) run through the very runners and gates the HIP kernels face
(tests/lora_cases.py) -- so a gate that cannot fail, or a runner with an indexing slip, shows here without a GPU."""
import pytest
import torch

import lora_cases as LC
import ref_lora as R_
import standin_lora

F64 = torch.float64


def _w_elementwise(w, n, r, rank_major):
    out = torch.empty((n, r), dtype=F64)
    for c in range(n):
        for j in range(r):
            out[c, j] = float(w[j, c]) if rank_major else float(w[c, j])
    return out


@pytest.mark.parametrize("rank_major", [True, False])
@pytest.mark.parametrize("r", [8, 16])
def test_reference_against_einsum(r, rank_major):
    g = torch.Generator().manual_seed(7)
    R, C, N, scale = 5, 24, 16, 1.5
    x = torch.randn((R + 1, C + 8), generator=g).to(LC.BF)
    wd = torch.randn(((r, C + 8) if rank_major else (C, r + 8)), generator=g).to(LC.BF)
    W = _w_elementwise(wd, C, r, rank_major)
    X = x[:R, :C].to(F64)
    t, st = R_.down_ref(x, wd, R, C, r, rank_major, scale)
    assert torch.allclose(t, scale * torch.einsum("ic,cj->ij", X, W), rtol=1e-13, atol=0)
    assert torch.allclose(st, scale * torch.einsum("ic,cj->ij", X.abs(), W.abs()), rtol=1e-13, atol=0)
    tt = torch.randn((R, r + 8), generator=g).to(LC.BF)
    wu = torch.randn(((r, N + 8) if rank_major else (N, r + 8)), generator=g).to(LC.BF)
    Wu = _w_elementwise(wu, N, r, rank_major)
    y0 = torch.randn((R, N + 8), generator=g).to(LC.BF)
    T = tt[:R, :r].to(F64)
    y, sy = R_.up_add_ref(tt, wu, y0, R, N, r, rank_major, scale)
    assert torch.allclose(y, y0[:, :N].to(F64) + scale * torch.einsum("ij,nj->in", T, Wu), rtol=1e-13, atol=1e-15)
    assert torch.allclose(sy, y0[:, :N].to(F64).abs() + scale * torch.einsum("ij,nj->in", T.abs(), Wu.abs()), rtol=1e-13, atol=0)
    gr, sg = R_.wgrad_ref(tt, x, R, C, r, scale)
    assert torch.allclose(gr, scale * torch.einsum("ij,ic->cj", T, X), rtol=1e-13, atol=1e-15)
    assert torch.allclose(sg, scale * torch.einsum("ij,ic->cj", T.abs(), X.abs()), rtol=1e-13, atol=0)


@pytest.mark.parametrize("c", LC.DOWN, ids=LC.case_id)
def test_standin_down(c):
    LC.run_down(standin_lora, c, "cpu")


@pytest.mark.parametrize("c", LC.UP_ADD, ids=LC.case_id)
def test_standin_up_add(c):
    LC.run_up_add(standin_lora, c, "cpu")


@pytest.mark.parametrize("c", LC.WGRAD, ids=LC.case_id)
def test_standin_wgrad(c):
    LC.run_wgrad(standin_lora, c, "cpu")


def test_gate_rejects_a_second_rounding():
    """a t rounded to bf16 BEFORE the scale (two roundings) must not pass the down gate at scale 1.5"""
    g = torch.Generator().manual_seed(3)
    R, C, r = 64, 256, 16
    x = torch.randn((R, C), generator=g).to(LC.BF)
    w = torch.randn((r, C), generator=g).to(LC.BF)
    ref, sc = R_.down_ref(x, w, R, C, r, True, 1.5)
    bad = ((x.double() @ w.double().t()).float().to(LC.BF).float() * 1.5).to(LC.BF)
    with pytest.raises(AssertionError):
        R_.close_scaled(bad, ref, sc, LC.GATES["down"], "twice rounded")
