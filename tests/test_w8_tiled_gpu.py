"""The many-row FP8 product on the GPU (include/mpv.h, "FP8 decoder weights": mpv_gemm_w8_tiled; csrc/gemm_w8.hip) and the decode
states whose steps have more than MPV_W8_MAX_ROWS rows: every code, exact arithmetic, random operands against the fp32 torch product
of the dequantised weight, the step's epilogues, row invariance, refusals, and FP8 states of 100 / 102 sequences against bf16 states
on the dequantised decoder -- and against the hybrid (original weights behind the dequantised embedding) that such steps ran before."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import w8_cases as wc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def bits(t):
    return t.view(torch.int16)


# ------------------------------------------------------------------------------------------------ 1. every code
def test_every_code_converts_exactly(dev):
    from youku_mplug_amd import ops
    a, codes, scale, want = wc.all_codes_case()
    got = ops.gemm_w8_tiled(a.to(dev), codes.to(dev), scale.to(dev), 2, 256, 64)
    bad = torch.nonzero(got.cpu().float() != want)
    assert bad.numel() == 0, bad[:8].tolist()
    nz = want != 0
    assert torch.equal(bits(got.cpu())[nz], bits(want.to(BF))[nz])                              # bit for bit


# ------------------------------------------------------------------------------------------------ 2. exact arithmetic
EXACT = [(97, 64, 8192), (160, 64, 8192), (512, 64, 8192), (101, 40, 1040), (512, 4096, 384), (160, 6144, 272), (500, 8200, 144),
         (500, 2048, 272)]


@pytest.mark.parametrize("M,N,K", EXACT, ids=lambda v: str(v))
def test_exact_product_is_the_bf16_rounding_of_the_fp64_result(dev, M, N, K):
    """every partial sum is exact in fp32 in any order (tests/test_w8_tiled_cpu.py checks the construction): a wrong lane, K step,
    LDS unit or row guard shows as a wrong bit.  (101, 40, 1040): guarded columns, a K tail, rows that fill no block.  The last four
    have enough columns for the host to give a workgroup several row blocks (the 64-column cases run one per workgroup): 4 blocks x
    128 columns, 2 x 128, 5 x 128 with the last workgroup cut at 8 columns, 4 x 64."""
    from youku_mplug_amd import ops
    a, codes, scale, want = wc.exact_case(M, N, K)
    got = ops.gemm_w8_tiled(a.to(dev), codes.to(dev), scale.to(dev), M, N, K).cpu()
    wb = want.to(BF)
    assert torch.equal(got.float(), wb.float()), torch.nonzero(got.float() != wb.float())[:8].tolist()
    nz = wb.float() != 0
    assert torch.equal(bits(got)[nz], bits(wb)[nz])


# ------------------------------------------------------------------------------------------------ 3. random operands
@functools.lru_cache(maxsize=None)
def _quantised(N, K, seed, dev):
    from youku_mplug_amd import ops
    _, w = wc.random_operands(1, N, K, seed, dev)
    codes, scale = ops.quantize_rows_e4m3(w)
    return codes, scale, wc.deq(codes, scale)


RANDOM = [(M, N, K) for N, K in ((24, 80), (256, 1024)) for M in (97, 160, 500)] + [(160, 2048, 8192), (160, 6144, 2048), (512, 6144, 2048)]


@pytest.mark.parametrize("M,N,K", RANDOM, ids=lambda v: str(v))
def test_random_product_against_fp32_torch_and_the_streaming_kernel(dev, M, N, K):
    from youku_mplug_amd import ops
    codes, scale, wd = _quantised(N, K, 9 if N >= 2048 else 7, dev)
    a, _ = wc.random_operands(M, 8, K, 100 + M, dev)
    got = ops.gemm_w8_tiled(a, codes, scale, M, N, K)
    err = rel(got, a.float() @ wd.t())
    other = rel(got, ops.gemm_w8(a, codes, scale, M, N, K))
    print(f"gemm_w8_tiled M={M} N={N} K={K}: {err:.3e} of the fp32 product, {other:.3e} of gemm_w8")
    assert err <= wc.GATE, err
    assert other <= wc.GATE, other


# ------------------------------------------------------------------------------------------------ 4. epilogues
@pytest.mark.parametrize("epi", ["bias", "bias_gelu", "bias_residual", "row_map"])
def test_epilogues_at_rows_that_are_no_multiple_of_16(dev, epi):
    from youku_mplug_amd import ops
    M, N, K = 101, 256, 1024
    codes, scale, wd = _quantised(N, K, 7, dev)
    a, _ = wc.random_operands(M, 8, K, 300, dev)
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(N, generator=g).to(BF).to(dev)
    z = a.float() @ wd.t() + bias.float()[None]
    if epi == "bias":
        got, want = ops.gemm_w8_tiled(a, codes, scale, M, N, K, bias=bias), z
    elif epi == "bias_gelu":
        got = ops.gemm_w8_tiled(a, codes, scale, M, N, K, bias=bias, act=ops.ACT_GELU_TANH)
        want = F.gelu(z.to(BF).float(), approximate="tanh")
    elif epi == "bias_residual":
        res = torch.randn(M, N + 8, generator=g).to(BF).to(dev)
        got = ops.gemm_w8_tiled(a, codes, scale, M, N, K, bias=bias, residual=res, ldr=N + 8)
        want = z + res[:, :N].float()
    else:                                                   # 15 sequences x 7 new rows (the last holds 3) at positions 2..8 of caches of 10 rows
        grp, stride, off = 7, 10, 2
        out = torch.full((15 * stride, N), 7.0, dtype=BF, device=dev)
        ops.gemm_w8_tiled(a, codes, scale, M, N, K, bias=bias, cmap=(grp, stride, off), out=out)
        rows = torch.tensor([(m // grp) * stride + m % grp + off for m in range(M)], device=dev)
        keep = torch.ones(15 * stride, dtype=torch.bool, device=dev)
        keep[rows] = False
        assert (out[keep] == 7.0).all()                     # the rows it must not touch
        got, want = out[rows], z
    err = rel(got, want)
    print(f"gemm_w8_tiled epilogue {epi}: {err:.3e}")
    assert err <= wc.GATE, err


# ------------------------------------------------------------------------------------------------ 5. row invariance
@pytest.mark.parametrize("N,K", [(256, 1024), (2048, 8192), (24, 80)], ids=lambda v: str(v))
def test_rows_do_not_depend_on_the_row_count_the_workspace_or_the_run(dev, N, K):
    from youku_mplug_amd import ops
    codes, scale, _ = _quantised(N, K, 9 if K == 8192 else 7, dev)
    a, _ = wc.random_operands(512, 8, K, 400, dev)
    bias = torch.linspace(-1, 1, N).to(BF).to(dev)
    kw = dict(bias=bias, act=ops.ACT_GELU_TANH)
    full = ops.gemm_w8_tiled(a, codes, scale, 512, N, K, **kw)
    again = ops.gemm_w8_tiled(a, codes, scale, 512, N, K, **kw)
    assert torch.equal(bits(full), bits(again))
    bare = ops.gemm_w8_tiled(a, codes, scale, 512, N, K, use_workspace=False, **kw)
    assert torch.equal(bits(full), bits(bare))
    for r0, n in ((0, 97), (352, 160), (511, 1), (17, 5)):
        part = ops.gemm_w8_tiled(a[r0:r0 + n].contiguous(), codes, scale, n, N, K, **kw)
        assert torch.equal(bits(part), bits(full[r0:r0 + n])), (r0, n)


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
            ops.gemm_w8_tiled(big, codes, scale, kw.pop("M", 16), kw.pop("N", N), kw.pop("K", K), out=out, lda=K, ldw=K, ldc=N, **kw, **other)
    rc = _lib.lib().mpv_gemm_w8_tiled(a.data_ptr(), None, scale.data_ptr(), out.data_ptr(), 16, N, K, K, K, N, None, None, 0, ops._stream())
    assert rc < 0
    torch.cuda.synchronize()
    assert (out == 3.0).all()


# ------------------------------------------------------------------------------------------------ 7. states above 96 rows
@functools.lru_cache(maxsize=None)
def _tiny(dev):
    """the tiny decoder, a copy with dequantized_state_dict() loaded (the function the FP8 states compute) and a copy with ONLY
    the dequantised embedding loaded (what steps above MPV_W8_MAX_ROWS rows ran before they reached the codes)"""
    from oracle.weights import CONFIG_TINY, make_state_dict
    from youku_mplug_amd.pretrain import synthetic_model
    cfg = CONFIG_TINY
    model = synthetic_model(cfg, device=dev)
    model.load_state_dict({k: v.to(BF) for k, v in make_state_dict(cfg, 6).items()}, strict=True)
    model.eval()
    gpt = model.text_decoder
    deq_sd = gpt.dequantized_state_dict()
    ref, hybrid = copy.deepcopy(gpt), copy.deepcopy(gpt)
    for twin in (ref, hybrid):
        twin.clear_decode_weights()
    ref.load_state_dict(deq_sd, strict=False)
    emb = [k for k in deq_sd if "word_embeddings" in k]
    assert len(emb) == 1
    hybrid.load_state_dict({emb[0]: deq_sd[emb[0]]}, strict=False)
    return cfg, gpt, ref, hybrid


def _rows():
    from youku_mplug_amd import _lib
    assert _lib.W8_TILED_MAX_ROWS >= 160
    return _lib.W8_MAX_ROWS + 4


def test_fp8_decode_state_above_the_streaming_limit_matches_the_dequantised_decoder(dev):
    """100 sequences: a prefill of 100 x 2 tokens (200 rows), three single steps (100 rows), a re-order, one more step.  Every
    logits tensor is within 1e-2 of the bf16 state on the dequantised decoder and is not the hybrid's."""
    from youku_mplug_amd.generation import DecodeState
    cfg, gpt, ref, hybrid = _tiny(dev)
    B = _rows()
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, cfg.vocab, (B, 6), generator=g).to(dev)
    s8, sd, sh = DecodeState(gpt, B, 8, "fp8"), DecodeState(ref, B, 8), DecodeState(hybrid, B, 8)
    assert s8.q8 is gpt._decode_weights_q8 and sd.q8 is None and sh.q8 is None
    outs = [tuple(s.step(ids[:, :2]) for s in (s8, sd, sh))]
    for t in range(2, 5):
        outs.append(tuple(s.step(ids[:, t:t + 1]) for s in (s8, sd, sh)))
    perm = torch.randperm(B, generator=g).to(dev)
    perm[1] = perm[0]
    for s in (s8, sd, sh):
        s.reorder(perm)
    outs.append(tuple(s.step(ids[perm, 5:6]) for s in (s8, sd, sh)))
    errs = [rel(a, b) for a, b, _ in outs]
    print("fp8 DecodeState of", B, "sequences vs the dequantised decoder:", " ".join(f"{e:.3e}" for e in errs),
          "; vs the hybrid:", " ".join(f"{rel(a, c):.3e}" for a, _, c in outs))
    assert max(errs) <= 1e-2, errs
    assert all(not torch.equal(a, c) for a, _, c in outs)


def test_fp8_shared_prefix_state_above_the_streaming_limit_matches_the_dequantised_decoder(dev):
    """34 groups x fan 3: a prefill of 34 x (8 + 4) = 408 rows, five steps of 102 rows with one re-order"""
    from youku_mplug_amd.generation import SharedPrefixDecodeState
    cfg, gpt, ref, hybrid = _tiny(dev)
    fan, Q, P, H = 3, 8, 4, cfg.hidden
    G = -(-_rows() // fan)
    g = torch.Generator().manual_seed(8)
    qe = (torch.randn(G, Q, H, generator=g) * 0.5).to(dev).to(BF)
    prompt = torch.randint(0, cfg.vocab, (G, P), generator=g).to(dev)
    s8, sd, sh = (SharedPrefixDecodeState(gpt, G * fan, Q + P + 6, "fp8"), SharedPrefixDecodeState(ref, G * fan, Q + P + 6),
                  SharedPrefixDecodeState(hybrid, G * fan, Q + P + 6))
    outs = [tuple(s.prefill_fan_out(prompt, qe, fan) for s in (s8, sd, sh))]
    for i in range(5):
        if i == 3:
            perm = (torch.arange(G * fan) // fan * fan + torch.randint(0, fan, (G * fan,), generator=g)).to(dev)     # within each group
            for s in (s8, sd, sh):
                s.reorder(perm)
        tok = torch.randint(0, cfg.vocab, (G * fan, 1), generator=g).to(dev)
        outs.append(tuple(s.step(tok) for s in (s8, sd, sh)))
    errs = [rel(a, b) for a, b, _ in outs]
    print("fp8 SharedPrefixDecodeState of", G * fan, "sequences vs the dequantised decoder:", " ".join(f"{e:.3e}" for e in errs),
          "; vs the hybrid:", " ".join(f"{rel(a, c):.3e}" for a, _, c in outs))
    assert max(errs) <= 1e-2, errs
    assert all(not torch.equal(a, c) for a, _, c in outs)
    assert s8.prefix.q8 is gpt._decode_weights_q8 and sd.prefix.q8 is None


# ------------------------------------------------------------------------------------------------ 8. the boundary
@pytest.mark.parametrize("extra", [0, 1])
def test_one_token_steps_on_both_sides_of_the_streaming_limit(dev, extra):
    from youku_mplug_amd import _lib
    from youku_mplug_amd.generation import DecodeState
    cfg, gpt, ref, _ = _tiny(dev)
    B = _lib.W8_MAX_ROWS + extra
    g = torch.Generator().manual_seed(11 + extra)
    ids = torch.randint(0, cfg.vocab, (B, 3), generator=g).to(dev)
    s8, sd = DecodeState(gpt, B, 4, "fp8"), DecodeState(ref, B, 4)
    errs = [rel(s8.step(ids[:, t:t + 1]), sd.step(ids[:, t:t + 1])) for t in range(3)]
    print(f"one-token steps at batch {B}:", " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) <= 1e-2, errs
