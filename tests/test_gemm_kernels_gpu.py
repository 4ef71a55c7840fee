"""The bf16 GEMM family -- csrc/gemm.hip (the 128x128 kernel with its tail split, the split-K weight-gradient pass and its reduce, the four
instances of the small-M weight-streaming kernel, the batched entry) and csrc/gemm256.hip (the 256 / 192 / 160-row eight-phase kernel in
its five operand instances, every epilogue kind, the weight-gradient and forward splits, row bands) -- against the fp64 reference of
tests/ref_gemm.py, element by element, at the smallest shapes that reach each instance and branch (the tables of tests/gemm_cases.py say
which and why).  Tolerances: gemm_cases.GATES (rtol from the number format, coefficient = 2 x the residual measured on an MI355X per
unit of the element's scale; pytest -s prints every comparison's worst residual; profiles/gemm_kernel_errors.md holds the table).
Everything called identical, dropped or untouched is compared on the raw bits.  Kernels are pinned with tile_hint / split_hint only.
Run on the MI355X box: pytest -m gpu tests/test_gemm_kernels_gpu.py"""
import ctypes as C

import pytest
import torch

import gemm_cases as G
import ref_gemm as R

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("name,c", G.SMALL_M_CASES, ids=_ids(G.SMALL_M_CASES))
def test_small_m_vs_fp64(dev, name, c):
    """gemm_small_m_kernel <true,16,8>, <true,4,8>, <true,4,16> and <false>: M in {1, 5, 16}, every K-loop shape, the epilogue of the
    decode steps (bias, activation, residual, padded ldc / ldr, the cmap that lands the qkv row in the KV cache)."""
    from youku_mplug_amd import ops
    G.run_gemm(ops, dev, c)


@pytest.mark.parametrize("name,c", G.K128_CASES, ids=_ids(G.K128_CASES))
def test_gemm128_vs_fp64(dev, name, c):
    """gemm_bf16_kernel in its three operand forms: ragged edges, odd-K weight gradients, split-K with its reduce, the tail split, every
    epilogue option singly and in the model's combinations."""
    from youku_mplug_amd import ops
    G.run_gemm(ops, dev, c)


@pytest.mark.parametrize("name,c", G.K256_CASES, ids=_ids(G.K256_CASES))
def test_gemm256_vs_fp64(dev, name, c):
    """gemm256_kernel: five operand instances, three tile heights, every epilogue kind of its dispatch, weight-gradient splits with a
    ragged last split, the forward split with bias and dropout in the reduce."""
    from youku_mplug_amd import ops
    G.run_gemm(ops, dev, c)


@pytest.mark.parametrize("form,batch,M,N,K", G.BATCHED)
def test_gemm_batched_vs_fp64(dev, form, batch, M, N, K):
    from youku_mplug_amd import ops
    G.run_batched(ops, dev, form, batch, M, N, K)


@pytest.mark.parametrize("entry", G.BANDS, ids=[b[0][0] for b in G.BANDS])
def test_row_bands_vs_fp64(dev, entry):
    """A product whose rows mpv_gemm256_try_launch cuts into two / three launches of different tile heights: the plan is asked from the
    hook with this device's CU count and must have the bands the table names on the 256 CUs of an MI355X (a single band there is a
    failure, not a skip); the product, with a residual and a scattering cmap, then goes through the same gates."""
    from youku_mplug_amd import _lib, ops
    (name, c), want, preact, ext = entry
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    out6 = (C.c_int * 6)()
    nb = _lib.lib().mpv_gemm_plan_bands(c["M"], c["N"], c["K"], ncu, preact, ext, out6)
    plan = tuple(out6[2 * i] for i in range(nb))
    assert nb > 1 or ncu != 256, f"{name}: a single band on {ncu} CUs"
    if ncu == 256:
        assert plan == want, f"{name}: plan {plan} on 256 CUs, the table says {want}"
    G.run_gemm(ops, dev, c)


def test_dropout_in_the_reduce_keeps_the_tile_epilogues_mask(dev):
    """The forward split drops in splitk_reduce_kernel, the unsplit product in the tile epilogue: same seed / offset / shape give the SAME
    mask (the element index is offset + m * N + n in both) and values within the gates of one reference.  The bits of kept elements are
    NOT promised equal: the split sums its K-parts in another order."""
    from youku_mplug_amd import ops
    split = dict(G.K256_CASES)["k256-fwdsplit-nt-256x256x4096-bias-drop"]
    whole = dict(split, path="k128_tail", tile_hint=128)          # same name -> same operands; four 128x128 tiles, each a tail split of 4 parts
    a = G.run_gemm(ops, dev, split)
    b = G.run_gemm(ops, dev, whole)
    keep = R.keep_mask(G.DROP_SEED, G.DROP_OFFSET, 256, 256, 0.1, device=dev)
    assert torch.equal(a[~keep], b[~keep]) and torch.equal(a == 0, b == 0)
