"""FP8 decoder weights on the host (include/mpv.h, "FP8 decoder weights"): the stand-in quantiser against the contract and torch's
float8_e4m3fn conversion, the constructions of the GPU tests, the library's exports and host-side refusals, and the plumbing of
decode_weights="fp8" through the generation loops on the stand-ins."""
import copy
import ctypes
import math

import pytest
import torch

import standin_w8 as sw
import w8_cases as wc

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ the quantiser
def test_standin_quantiser_follows_the_contract():
    w = wc.quantiser_rows()
    codes, scale = sw.quantize_rows_e4m3(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (7,)
    for n in range(w.shape[0]):
        amax = float(w[n].float().abs().max())
        e = wc.exponent_of(amax)
        assert float(scale[n]) == math.ldexp(1.0, e), n
        if amax > 0:
            assert amax <= 448.0 * 2.0 ** e and amax > 448.0 * 2.0 ** (e - 1), n      # the smallest such exponent
        want = (w[n].float() / float(scale[n])).to(torch.float8_e4m3fn).view(torch.uint8)
        assert torch.equal(codes[n], want), n                                          # torch's conversion of w / scale
    assert float(scale[3]) == 1.0 and not codes[3].any()                               # the zero row
    assert float(scale[4]) == 2.0 ** -3 and wc.CODE_VALUE[codes[4, 5].long()] == -448.0  # amax exactly 448 * 2^e: the largest code
    assert float(scale[5]) == 2.0 ** -2                                                # one bf16 step above: the exponent moves up
    assert codes[6, 1] == 0x80                                                         # -0.0 keeps its sign
    assert not ((codes & 0x7f) == 0x7f).any()                                          # no NaN code
    d = wc.deq(codes, scale)
    assert d.abs().max() <= w.float().abs().max() and torch.equal(d.to(BF).float(), d)  # deq * scale is a bf16 number
    # the rounding error of a Gaussian row: about 2.7 % relative L2 (what the docs quote)
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(64, 2048, generator=g) * 0.02).to(BF)
    c, s = sw.quantize_rows_e4m3(x)
    err = ((wc.deq(c, s) - x.float()).norm() / x.float().norm()).item()
    assert 0.02 < err < 0.035, err
    with pytest.raises(ValueError):
        sw.quantize_rows_e4m3(torch.zeros(8, 24, dtype=BF))                            # K % 16


def test_standin_quantiser_takes_a_row_pitch():
    g = torch.Generator().manual_seed(1)
    big = torch.randn(24, 104, generator=g).to(BF)
    c0, s0 = sw.quantize_rows_e4m3(big[:, :80].contiguous())
    c1, s1 = sw.quantize_rows_e4m3(big[:, :80])
    assert torch.equal(c0, c1) and torch.equal(s0, s1)


def test_all_codes_case_holds_every_finite_code():
    a, codes, scale, want = wc.all_codes_case()
    assert sorted(set(codes.view(-1).tolist())) == [b for b in range(256) if (b & 0x7f) != 0x7f]
    assert torch.isfinite(want).all() and want[0].abs().max() == 448.0 and (want[0] == 2.0 ** -9).any()     # the smallest subnormal
    assert torch.equal(want.to(BF).float(), want)                                      # every expected value is a bf16 number
    got = sw.gemm_w8(a, codes, scale, 2, 256, 64)
    assert torch.equal(got.float(), want)


@pytest.mark.parametrize("M", wc.EXACT_M)
def test_exact_case_is_exact_in_fp32_in_any_order(M):
    a, codes, scale, want = wc.exact_case(M, K=1024 if M > 1 else 8192)
    w32 = codes.view(torch.float8_e4m3fn).float()
    perm = torch.randperm(a.shape[1], generator=torch.Generator().manual_seed(M))
    s = torch.zeros(M, 64)
    for k in perm.tolist()[:4096]:                                                     # a sequential fp32 sum in a shuffled order
        s += a[:, k:k + 1].float() * w32[None, :, k]
    full = (a[:, perm[:4096]].double() @ w32[:, perm[:4096]].double().t())
    assert torch.equal(s.double(), full)
    assert torch.equal((a.float() @ w32.t()).double() * scale.double()[None], want)    # torch's own fp32 order
    assert want.abs().max() < 2.0 ** 21


# ------------------------------------------------------------------------------------------------ the library on the host
NEW_SYMBOLS = ("mpv_quantize_rows_e4m3", "mpv_gemm_w8", "mpv_gpt_embed_w8_fwd", "mpv_gpt_decode_step_q8", "mpv_gpt_decode_step_shared_q8")


def test_library_exports_the_fp8_entries_and_refuses_on_the_host():
    """every refusal is a negative code from host-side checks: no device is needed (and none is touched) to get it"""
    from youku_mplug_amd import _lib
    lib = _lib.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(lib, sym)
    A, W, S, Cc = 0x10000, 0x20000, 0x30000, 0x40000                                   # never dereferenced on the host
    good = dict(A=A, W=W, S=S, C=Cc, M=5, N=64, K=128, lda=128, ldw=128, ldc=64)

    def call(ep=None, **over):
        a = dict(good, **over)
        return lib.mpv_gemm_w8(a["A"], a["W"], a["S"], a["C"], a["M"], a["N"], a["K"], a["lda"], a["ldw"], a["ldc"],
                               None if ep is None else ctypes.byref(ep), None)
    for over, code in ((dict(M=0), -1), (dict(M=513), -1), (dict(K=120), -1), (dict(N=60), -1), (dict(K=0), -1), (dict(lda=64), -1),
                       (dict(ldc=56), -1), (dict(A=None), -5), (dict(W=None), -5), (dict(S=None), -5), (dict(C=None), -5),
                       (dict(A=A + 8), -2), (dict(ldw=136), -2)):
        assert call(**over) == code, over
        assert b"mpv_gemm_w8" in lib.mpv_last_error()
    for field, value in (("out_f32", 1), ("accumulate", 1), ("act", 1), ("act", 3), ("a_group", 2), ("k_group", 2), ("preact_out", 0x50000),
                         ("act_bwd_z", 0x50000), ("dropout_p", 0.1), ("alpha", 2.0), ("alpha_dev", 0x50000), ("colsum_out", 0x50000),
                         ("row_tap_out", 0x50000), ("tile_hint", 128), ("colscale_cols", 8), ("keep_output", 1), ("preact_deriv", 1)):
        ep = _lib.GemmEpilogue()
        setattr(ep, field, value)
        assert call(ep) == -5, field
    assert lib.mpv_quantize_rows_e4m3(None, 8, 16, 16, W, S, None) == -5
    assert lib.mpv_quantize_rows_e4m3(A, 8, 24, 24, W, S, None) == -1
    assert lib.mpv_quantize_rows_e4m3(A, 8, 32, 16, W, S, None) == -1
    assert lib.mpv_quantize_rows_e4m3(A, 0, 32, 32, W, S, None) == -1
    w = _lib.GptWeights()
    w.layers = 2
    q8 = _lib.GptWeightsQ8()
    q8.layers = 1
    assert lib.mpv_gpt_decode_step_q8(ctypes.byref(w), None, None, 1, 8, 0, None, 0, None, 1, None, 0, None, None) == -5
    assert lib.mpv_gpt_decode_step_q8(ctypes.byref(w), ctypes.byref(q8), None, 1, 8, 0, None, 0, None, 1, None, 0, None, None) == -5
    assert b"mpv_gpt_decode_step_q8" in lib.mpv_last_error()
    assert lib.mpv_gpt_decode_step_shared_q8(ctypes.byref(w), ctypes.byref(q8), None, None, 1, 1, 4, 4, 0, None, None, 0, None, None) == -5
    assert b"mpv_gpt_decode_step_shared_q8" in lib.mpv_last_error()
    assert ctypes.sizeof(_lib.GptLayerWeightsQ8) == 64 and ctypes.sizeof(_lib.GptWeightsQ8) == 32


def test_header_and_binding_agree_on_the_row_limit():
    import os
    import re
    from youku_mplug_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mpv.h")).read()
    assert int(re.search(r"#define MPV_W8_MAX_ROWS (\d+)", text).group(1)) == _lib.W8_MAX_ROWS


# ------------------------------------------------------------------------------------------------ the loops on the stand-ins
def _on_cpu(monkeypatch):
    import test_beam_groups_cpu as tbg
    dev = tbg._on_cpu(monkeypatch)
    sw.install(monkeypatch)
    return dev


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_generate_fp8_equals_the_dequantised_model_on_standins(monkeypatch):
    """decode_weights="fp8" against the default path on a copy of the model with dequantized_state_dict() loaded: on the stand-ins
    both are the same fp32 function, so tokens AND scores are equal -- per-clip beam search, lockstep beam search, group beams and
    sampling with return_scores, both KV modes.  The default and "bf16" leave no DecodeWeightsQ8 behind; bad values raise."""
    import caption_score_cases as cs
    from youku_mplug_amd import generation
    dev = _on_cpu(monkeypatch)
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    gpt = model.text_decoder
    term = g["meta"]["eod_id"]
    sel = [0, 1, 0]
    text = cs.text_of(ids, mask, sel, dev)
    vid = video[sel].to(BF)
    cases = [dict()]
    for kv in ("per_sequence", "shared_prefix"):
        cases += [dict(batched=True, kv_cache=kv),
                  dict(batched=True, kv_cache=kv, beam_groups=2, diversity_penalty=1.5, beam_size=3, num_return_gen=4),
                  dict(do_sample=True, num_samples=3, seed=5, temperature=1.2, top_p=0.9, return_scores=True, kv_cache=kv)]
    plain = [model.generate(vid, text, termination_id=term, **kw) for kw in cases[:2]]
    assert "_decode_weights_q8" not in gpt.__dict__                                    # the default leaves nothing behind
    explicit = model.generate(vid, text, termination_id=term, decode_weights="bf16", **cases[1])
    assert "_decode_weights_q8" not in gpt.__dict__ and _same(explicit, plain[1])
    twin = copy.deepcopy(model)
    deq_sd = gpt.dequantized_state_dict()                                              # quantises
    assert isinstance(gpt._decode_weights_q8, generation.DecodeWeightsQ8)
    own = gpt.state_dict()
    assert len(deq_sd) == 4 * cfg.layers + 1 and all(k in own and own[k].shape == v.shape and v.dtype == BF for k, v in deq_sd.items())
    assert any(not torch.equal(own[k], v) for k, v in deq_sd.items())
    twin.text_decoder.load_state_dict(deq_sd, strict=False)
    made = []
    orig = generation.DecodeState.__init__

    def spy(self, *a, **kw):
        orig(self, *a, **kw)
        made.append(self.q8)
    monkeypatch.setattr(generation.DecodeState, "__init__", spy)
    for kw in cases:
        made.clear()
        want = twin.generate(vid, text, termination_id=term, **kw)
        assert made and all(q is None for q in made), kw                               # the twin runs on its bf16 weights
        made.clear()
        got = model.generate(vid, text, termination_id=term, decode_weights="fp8", **kw)
        assert made and all(q is gpt._decode_weights_q8 for q in made), kw             # every state took the ONE quantised copy
        assert _same(got, want), kw
    assert "_decode_weights_q8" not in twin.text_decoder.__dict__
    for bad in ("fp16", "int8", None, 8):
        with pytest.raises(ValueError, match="decode_weights"):
            model.generate(vid, text, termination_id=term, decode_weights=bad)
        for call in (lambda: gpt.beam_search_batched(ids[:1, :3], decode_weights=bad), lambda: gpt.sample_batched(ids[:1, :3], decode_weights=bad),
                     lambda: gpt.generate(ids[:1, :3], decode_weights=bad), lambda: gpt.beam_search(ids[:1, :3], decode_weights=bad),
                     lambda: gpt.sample(ids[:1, :3], decode_weights=bad), lambda: generation.make_state_fn(gpt, weights=bad)):
            with pytest.raises(ValueError, match="decode_weights"):
                call()
    gpt.clear_decode_weights()
    assert "_decode_weights_q8" not in gpt.__dict__
    gpt.clear_decode_weights()                                                         # nothing to clear: no error


def test_an_in_place_weight_edit_is_picked_up_by_the_next_state(monkeypatch):
    import test_decode_shared_cpu as tds
    from youku_mplug_amd.generation import DecodeState, SharedPrefixDecodeState
    sw.install(monkeypatch)
    cfg, gpt = tds._tiny_decoder(torch.device("cpu"))
    q8 = gpt.quantize_decode_weights()
    assert not q8.stale() and gpt.decode_weights_q8() is q8
    st = DecodeState(gpt, 2, 8, "fp8")
    assert st.q8 is q8
    tok = torch.tensor([[3, 4], [5, 6]])
    before = st.step(tok)
    w = gpt.dist_model.language_model.encoder.layers[1].mlp.dense_4h_to_h.weight
    with torch.no_grad():
        w.mul_(-1.5)
    assert q8.stale()
    st2 = DecodeState(gpt, 2, 8, "fp8")
    assert st2.q8 is not q8 and st2.q8 is gpt._decode_weights_q8 and not st2.q8.stale()
    after = st2.step(tok)
    assert not torch.equal(before, after)
    ref = copy.deepcopy(gpt)
    ref.clear_decode_weights()
    ref.load_state_dict(gpt.dequantized_state_dict(), strict=False)
    assert torch.equal(DecodeState(ref, 2, 8).step(tok), after)
    sh = SharedPrefixDecodeState(gpt, 4, 8, "fp8")
    sh.prefill_fan_out(tok, None, 2)
    assert sh.prefix.q8 is st2.q8
    with pytest.raises(ValueError, match="decode_weights"):
        SharedPrefixDecodeState(gpt, 4, 8, "fp4")
    assert q8.nbytes() == sum(p.numel() + 4 * p.shape[0] for p in q8.sources)
