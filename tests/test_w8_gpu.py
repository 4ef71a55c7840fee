"""FP8 decoder weights on the GPU (include/mpv.h, "FP8 decoder weights"; csrc/gemm_w8.hip): the quantiser against the stand-in, the
conversion of every code, an exact-arithmetic product, random products against the fp32 torch product of the dequantised weight
with every epilogue of the decode step, row invariance, refusals, and the FP8 decode states against bf16 states on the dequantised
decoder."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import standin_w8 as sw
import w8_cases as wc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


# ------------------------------------------------------------------------------------------------ 1. the quantiser
@pytest.mark.parametrize("N,K,pad", wc.QUANT_SHAPES, ids=lambda v: str(v))
def test_quantiser_matches_the_standin(dev, N, K, pad):
    from youku_mplug_amd import ops
    g = torch.Generator().manual_seed(N + K)
    big = (torch.randn(N, K + pad, generator=g) * torch.logspace(-5, 1, N)[:, None]).to(BF)     # rows of many magnitudes
    big[N // 2] = 0                                                                             # a zero row
    big[1, :16] = wc.quantiser_rows(16)[4]                                                      # amax exactly 448 * 2^e ...
    big[1, 16:] = 0
    if N > 2:
        big[2, :16] = wc.quantiser_rows(16)[6]                                                  # ... and a -0.0
        big[2, 16:] = 0
    w = big[:, :K]
    want_c, want_s = sw.quantize_rows_e4m3(w)
    codes, scale = ops.quantize_rows_e4m3(big.to(dev)[:, :K])
    assert codes.shape == (N, K) and codes.dtype == torch.uint8 and scale.dtype == torch.float32
    assert torch.equal(scale.cpu(), want_s)
    assert not ((codes & 0x7f) == 0x7f).any()
    assert torch.equal(wc.deq(codes.cpu(), scale.cpu()), wc.deq(want_c, want_s))                # as floats: +-0 compare equal


# ------------------------------------------------------------------------------------------------ 2. every code
def test_every_code_converts_exactly(dev):
    from youku_mplug_amd import ops
    a, codes, scale, want = wc.all_codes_case()
    got = ops.gemm_w8(a.to(dev), codes.to(dev), scale.to(dev), 2, 256, 64)
    bad = torch.nonzero(got.cpu().float() != want)
    assert bad.numel() == 0, bad[:8].tolist()
    nz = want != 0
    assert torch.equal(got.cpu().view(torch.int16)[nz], want.to(BF).view(torch.int16)[nz])      # bit for bit


# ------------------------------------------------------------------------------------------------ 3. exact arithmetic
@pytest.mark.parametrize("M", wc.EXACT_M)
def test_exact_product_is_the_bf16_rounding_of_the_fp64_result(dev, M):
    """every partial sum is exact in fp32 in any order (tests/test_w8_cpu.py checks the construction): a wrong lane, K slice or
    reduce shows as a wrong bit"""
    from youku_mplug_amd import ops
    a, codes, scale, want = wc.exact_case(M)
    got = ops.gemm_w8(a.to(dev), codes.to(dev), scale.to(dev), M, 64, 8192).cpu()
    wb = want.to(BF)
    assert torch.equal(got.float(), wb.float()), torch.nonzero(got.float() != wb.float())[:8].tolist()
    nz = wb.float() != 0
    assert torch.equal(got.view(torch.int16)[nz], wb.view(torch.int16)[nz])


# ------------------------------------------------------------------------------------------------ 4. random operands
@functools.lru_cache(maxsize=None)
def _quantised(N, K, seed, dev):
    from youku_mplug_amd import ops
    _, w = wc.random_operands(1, N, K, seed, dev)
    codes, scale = ops.quantize_rows_e4m3(w)
    return codes, scale, wc.deq(codes, scale)


@pytest.mark.parametrize("N,K", wc.SWEEP_NK, ids=lambda v: str(v))
@pytest.mark.parametrize("M", wc.SWEEP_M)
def test_random_product_against_fp32_torch(dev, M, N, K):
    from youku_mplug_amd import ops
    codes, scale, wd = _quantised(N, K, 7, dev)
    a, _ = wc.random_operands(M, 8, K, 100 + M, dev)
    got = ops.gemm_w8(a, codes, scale, M, N, K)
    err = rel(got, a.float() @ wd.t())
    print(f"gemm_w8 M={M} N={N} K={K}: {err:.3e}")
    assert err <= wc.GATE, err


@pytest.mark.parametrize("M,N,K", wc.LARGE, ids=lambda v: str(v))
def test_random_product_large_shapes(dev, M, N, K):
    from youku_mplug_amd import ops
    codes, scale, wd = _quantised(N, K, 9, dev)
    a, _ = wc.random_operands(M, 8, K, 200 + M, dev)
    got = ops.gemm_w8(a, codes, scale, M, N, K)
    err = rel(got, a.float() @ wd.t())
    print(f"gemm_w8 M={M} N={N} K={K}: {err:.3e}")
    assert err <= wc.GATE, err


@pytest.mark.parametrize("epi", ["bias", "bias_gelu", "bias_residual", "row_map"])
def test_epilogues_at_rows_that_are_no_multiple_of_16(dev, epi):
    from youku_mplug_amd import ops
    M, N, K = 21, 256, 1024
    codes, scale, wd = _quantised(N, K, 7, dev)
    a, _ = wc.random_operands(M, 8, K, 300, dev)
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(N, generator=g).to(BF).to(dev)
    z = a.float() @ wd.t() + bias.float()[None]
    if epi == "bias":
        got, want = ops.gemm_w8(a, codes, scale, M, N, K, bias=bias), z
    elif epi == "bias_gelu":
        got = ops.gemm_w8(a, codes, scale, M, N, K, bias=bias, act=ops.ACT_GELU_TANH)
        want = F.gelu(z.to(BF).float(), approximate="tanh")
    elif epi == "bias_residual":
        res = torch.randn(M, N + 8, generator=g).to(BF).to(dev)
        got = ops.gemm_w8(a, codes, scale, M, N, K, bias=bias, residual=res, ldr=N + 8)
        want = z + res[:, :N].float()
    else:                                                   # 3 sequences x 7 new rows at positions 2..8 of caches of 10 rows
        grp, stride, off = 7, 10, 2
        out = torch.full((3 * stride, N), 7.0, dtype=BF, device=dev)
        ops.gemm_w8(a, codes, scale, M, N, K, bias=bias, cmap=(grp, stride, off), out=out)
        rows = torch.tensor([(m // grp) * stride + m % grp + off for m in range(M)], device=dev)
        keep = torch.ones(3 * stride, dtype=torch.bool, device=dev)
        keep[rows] = False
        assert (out[keep] == 7.0).all()                     # the rows it must not touch
        got, want = out[rows], z
    err = rel(got, want)
    print(f"gemm_w8 epilogue {epi}: {err:.3e}")
    assert err <= wc.GATE, err


# ------------------------------------------------------------------------------------------------ 5. row invariance
@pytest.mark.parametrize("N,K", [(256, 1024), (2048, 8192), (24, 80)], ids=lambda v: str(v))
def test_rows_do_not_depend_on_the_row_count_and_runs_repeat(dev, N, K):
    from youku_mplug_amd import ops
    codes, scale, _ = _quantised(N, K, 9 if K == 8192 else 7, dev)
    a, _ = wc.random_operands(160, 8, K, 400, dev)
    bias = torch.linspace(-1, 1, N).to(BF).to(dev)
    full = ops.gemm_w8(a, codes, scale, 160, N, K, bias=bias, act=ops.ACT_GELU_TANH)
    again = ops.gemm_w8(a, codes, scale, 160, N, K, bias=bias, act=ops.ACT_GELU_TANH)
    assert torch.equal(full.view(torch.int16), again.view(torch.int16))
    for r0, n in ((0, 5), (155, 5), (17, 1), (159, 1), (128, 32)):
        part = ops.gemm_w8(a[r0:r0 + n].contiguous(), codes, scale, n, N, K, bias=bias, act=ops.ACT_GELU_TANH)
        assert torch.equal(part.view(torch.int16), full[r0:r0 + n].view(torch.int16)), (r0, n)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_c_untouched(dev):
    from youku_mplug_amd import _lib, ops
    N, K = 64, 128
    codes, scale, _ = _quantised(N, K, 7, dev)
    a, _ = wc.random_operands(16, 8, K, 1, dev)
    big = torch.zeros(520, K, dtype=BF, device=dev)
    out = torch.full((520, N), 3.0, dtype=BF, device=dev)
    for kw in (dict(M=0), dict(M=513), dict(K=120), dict(N=60), dict(other=dict(out_f32=1)), dict(other=dict(act_bwd=2)), dict(act=ops.ACT_GELU_ERF)):
        kw = dict(kw)
        other = kw.pop("other", {})
        with pytest.raises(_lib.MpvError):
            ops.gemm_w8(big, codes, scale, kw.pop("M", 16), kw.pop("N", N), kw.pop("K", K), out=out, lda=K, ldw=K, ldc=N, **kw, **other)
    rc = _lib.lib().mpv_gemm_w8(a.data_ptr(), None, scale.data_ptr(), out.data_ptr(), 16, N, K, K, K, N, None, ops._stream())
    assert rc < 0
    torch.cuda.synchronize()
    assert (out == 3.0).all()


# ------------------------------------------------------------------------------------------------ 7. the tiny decoder
def _tiny(dev):
    from oracle.weights import CONFIG_TINY, make_state_dict
    from youku_mplug_amd.pretrain import synthetic_model
    cfg = CONFIG_TINY
    model = synthetic_model(cfg, device=dev)
    model.load_state_dict({k: v.to(BF) for k, v in make_state_dict(cfg, 6).items()}, strict=True)
    model.eval()
    gpt = model.text_decoder
    ref = copy.deepcopy(gpt)
    ref.load_state_dict(gpt.dequantized_state_dict(), strict=False)
    assert "_decode_weights_q8" not in ref.__dict__
    return cfg, gpt, ref


def test_fp8_decode_state_matches_the_dequantised_decoder(dev):
    """test_kv_cache_decode_matches_full_forward's sequence -- a prefill of 3 x (8 + 4) rows, three single steps, a re-order, two
    steps -- on an FP8 DecodeState against a bf16 DecodeState on a copy with dequantized_state_dict() loaded (the same function:
    that test's 1e-2) and against the bf16 decoder's own logits (a different function: printed, and not equal)."""
    from youku_mplug_amd.generation import DecodeState
    cfg, gpt, ref = _tiny(dev)
    B, Q, L, H = 3, 8, 9, cfg.hidden
    g = torch.Generator().manual_seed(4)
    qe = (torch.randn(B, Q, H, generator=g) * 0.5).to(dev).to(BF)
    ids = torch.randint(0, cfg.vocab, (B, L), generator=g).to(dev)
    s8, sd, so_ = DecodeState(gpt, B, Q + L + 2, "fp8"), DecodeState(ref, B, Q + L + 2), DecodeState(gpt, B, Q + L + 2)
    assert s8.q8 is gpt._decode_weights_q8 and sd.q8 is None and so_.q8 is None
    worst, quant = 0.0, 0.0

    def step(tok, q=None):
        nonlocal worst, quant
        a, b, c = s8.step(tok, q), sd.step(tok, q), so_.step(tok, q)
        assert rel(a, b) <= 1e-2, rel(a, b)
        assert not torch.equal(a, c)                                   # the FP8 path was taken
        worst, quant = max(worst, rel(a, b)), max(quant, rel(a, c))
    step(ids[:, :4], qe)
    for t in range(4, 7):
        step(ids[:, t:t + 1])
    perm = torch.tensor([2, 0, 0], device=dev)
    for s in (s8, sd, so_):
        s.reorder(perm)
    ids2 = ids[perm]
    for t in range(7, 9):
        step(ids2[:, t:t + 1])
    print(f"fp8 DecodeState vs bf16 state on the dequantised decoder: {worst:.3e}; vs the bf16 decoder's own logits (quantisation): {quant:.3e}")


def test_fp8_shared_prefix_state_matches_the_dequantised_decoder(dev):
    from youku_mplug_amd.generation import SharedPrefixDecodeState
    cfg, gpt, ref = _tiny(dev)
    G, fan, Q, P, H = 2, 3, 8, 4, cfg.hidden
    g = torch.Generator().manual_seed(8)
    qe = (torch.randn(G, Q, H, generator=g) * 0.5).to(dev).to(BF)
    prompt = torch.randint(0, cfg.vocab, (G, P), generator=g).to(dev)
    s8, sd, so_ = (SharedPrefixDecodeState(gpt, G * fan, Q + P + 6, "fp8"), SharedPrefixDecodeState(ref, G * fan, Q + P + 6),
                   SharedPrefixDecodeState(gpt, G * fan, Q + P + 6))
    outs = [tuple(s.prefill_fan_out(prompt, qe, fan) for s in (s8, sd, so_))]
    for i in range(5):
        if i == 3:
            perm = torch.tensor([0, 0, 2, 5, 3, 3], device=dev)
            for s in (s8, sd, so_):
                s.reorder(perm)
        tok = torch.randint(0, cfg.vocab, (G * fan, 1), generator=g).to(dev)
        outs.append(tuple(s.step(tok) for s in (s8, sd, so_)))
    worst = max(rel(a, b) for a, b, _ in outs)
    quant = max(rel(a, c) for a, _, c in outs)
    print(f"fp8 SharedPrefixDecodeState vs bf16 state on the dequantised decoder: {worst:.3e}; vs the bf16 decoder's own (quantisation): {quant:.3e}")
    assert worst <= 1e-2, worst
    assert all(not torch.equal(a, c) for a, _, c in outs)
    assert s8.prefix.q8 is gpt._decode_weights_q8 and sd.prefix.q8 is None


# ------------------------------------------------------------------------------------------------ 8. the caption wrapper
def test_caption_generate_on_fp8_weights_is_well_formed(dev):
    import caption_score_cases as cs
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    term = g["meta"]["eod_id"]
    sel = [0, 1, 0]
    text = cs.text_of(ids, mask, sel, dev)
    vid = video[sel].to(dev).to(BF)
    Lt = ids.shape[1] + g["meta"]["tokens_to_generate"]
    res = model.generate(vid, text, termination_id=term, batched=True, kv_cache="shared_prefix", decode_weights="fp8")
    assert len(res) == 3
    for i, r in enumerate(res):
        pl = int(mask[sel[i]].sum()) - 1
        assert r.dim() == 2 and r.shape[0] >= 1 and r.shape[1] <= Lt and (r[:, :pl] == ids[sel[i], :pl]).all()
        assert ((r >= 0) & (r < cfg.vocab)).all()
    assert torch.equal(res[0], res[2])                                 # the same clip twice
    res, scores = model.generate(vid, text, termination_id=term, do_sample=True, num_samples=3, seed=5, temperature=1.2, top_p=0.9,
                                 return_scores=True, decode_weights="fp8")
    assert len(res) == len(scores) == 3
    for i, (r, sc) in enumerate(zip(res, scores)):
        pl = int(mask[sel[i]].sum()) - 1
        assert r.shape == (3, Lt) and (r[:, :pl] == ids[sel[i], :pl]).all()
        assert torch.isfinite(sc["sum_logprob"]).all() and (sc["count"] >= 1).all() and (sc["sum_logprob"] <= 0).all()
    assert model.text_decoder._decode_weights_q8 is not None
