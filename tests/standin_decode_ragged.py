"""Torch stand-ins of the ragged shared-prefix decode path (include/mpv.h: mpv_attn_decode_shared_ragged_fwd, mpv_gpt_prefill_ragged,
mpv_gpt_decode_step_shared_ragged and their _q8 forms) on host tensors, test-only: the attention with a prefix length per group (the
reference of the kernel's GPU test: per group, the fp32 softmax of tests/standin_decode_shared.py at that group's length), the
prefill of right-padded prompts with the LM head on each sequence's own last row, and the step behind
generation.SharedPrefixDecodeState once prefill_fan_out was given prompt_len.  install() adds them to the stand-ins of
tests/standin_w8.py (which include those of standin_decode_shared.py and standin_ops.py)."""
import math

import torch

import standin_decode_shared as sds
import standin_ops as so
import standin_w8 as sw

BF = torch.bfloat16


def _at(t, elements):
    """the buffer behind t from `elements` elements past t's first one (the stand-ins address operands from their storage offset)"""
    return t.as_strided((1,), (1,), t.storage_offset() + elements)


def attn_decode_shared_ragged_ref(q, k, v, pk, pv, lay, prefix_lay, n_seq, group_size, heads, lengths, own_len, hd, scale):
    """fp32: group g's sequences attend to the first lengths[g] rows of their prefix and to their own_len own rows -> [n_seq, heads, hd].
    Every group is attn_decode_shared_ref on that group alone with prefix_len = its length: nothing at or beyond a length is read."""
    out = []
    (pks, _, _), (pvs, _, _) = prefix_lay
    for g, plen in enumerate(lengths):
        s0 = g * group_size
        n = min(group_size, n_seq - s0)
        out.append(sds.attn_decode_shared_ref(_at(q, s0 * lay.q[0]), _at(k, s0 * lay.k[0]), _at(v, s0 * lay.v[0]), _at(pk, g * pks),
                                              _at(pv, g * pvs), lay, prefix_lay, n, group_size, heads, int(plen), own_len, hd, scale))
    return torch.cat(out, dim=0)


def ragged_prefill(self, tokens, query_embeds, prompt_len):
    """mpv_gpt_prefill_ragged / _q8 behind SharedPrefixDecodeState._ragged_prefill: standin_ops.decode_step at pos0 = 0 over the
    right-padded prompts, with the final norm and the LM head on row Q + prompt_len[b] - 1 of every sequence"""
    st = self.prefix
    real = st.gpt
    if st.q8 is not None:
        st.gpt = sw._dequantised_decoder(st.gpt, st.q8)
    try:
        lm = st.gpt.dist_model.language_model
        B, H, np_, hn, V, ML = st.batch, st.H, st.np_, st.hn, st.V, st.max_len
        lens = [int(x) for x in (prompt_len.tolist() if torch.is_tensor(prompt_len) else prompt_len)]
        qf = None if query_embeds is None else query_embeds.reshape(-1, H).to(BF).contiguous()
        Q = 0 if qf is None else qf.shape[0] // B
        L = tokens.shape[1]
        n = Q + L
        if len(lens) != B or min(lens) < 1 or max(lens) > L:
            raise ValueError("prompt_len out of range")
        assert st.pos == 0 and n <= ML and n <= lm.embedding.position_embeddings.weight.shape[0]
        self.group_prefix_len = torch.tensor([Q + x for x in lens], dtype=torch.int32)
        h = torch.empty((B, n, H), dtype=torch.float32)
        if Q:
            h[:, :Q] = qf.float().view(B, Q, H)
        h[:, Q:] = lm.embedding.word_embeddings.weight.float()[tokens]
        h = (h + lm.embedding.position_embeddings.weight.float()[:n][None]).to(BF).view(B * n, H)
        cs = (ML * 3 * H, 3 * hn, 3 * H)
        lay = so.AttnLayout(cs, cs, cs, (n * H, hn, H))
        for li, layer in enumerate(lm.encoder.layers):
            att, mlp, cache = layer.self_attention, layer.mlp, st.cache[li]
            x1, _, _ = so.layernorm_fwd(h, layer.input_layernorm.weight, layer.input_layernorm.bias, layer.input_layernorm.eps, B * n, H)
            so.gemm(x1, att.query_key_value.weight, B * n, 3 * H, H, bias=att.query_key_value.bias, cmap=(n, ML, 0), out=cache)
            ctx = torch.zeros((B * n, H), dtype=BF)
            so.attn_fwd(cache, cache[:, hn:], cache[:, 2 * hn:], ctx, lay, B, np_, n, n, hn, causal=True, scale=1.0 / math.sqrt(hn))
            h1 = so.gemm(ctx, att.dense.weight, B * n, H, H, bias=att.dense.bias, residual=h)
            x2, _, _ = so.layernorm_fwd(h1, layer.post_attention_layernorm.weight, layer.post_attention_layernorm.bias,
                                        layer.post_attention_layernorm.eps, B * n, H)
            F4 = mlp.dense_h_to_4h.out_features
            g = so.gemm(x2, mlp.dense_h_to_4h.weight, B * n, F4, H, bias=mlp.dense_h_to_4h.bias, act=so.ACT_GELU_TANH)
            h = so.gemm(g, mlp.dense_4h_to_h.weight, B * n, H, F4, bias=mlp.dense_4h_to_h.bias, residual=h1)
        rows = torch.tensor([b * n + Q + x - 1 for b, x in enumerate(lens)])
        last = so.gather_rows(h, rows, B, H)
        fl = lm.encoder.final_layernorm
        xf, _, _ = so.layernorm_fwd(last, fl.weight, fl.bias, fl.eps, B, H)
        st.pos += n
        return so.gemm(xf, lm.embedding.word_embeddings.weight, B, V, H)
    finally:
        st.gpt = real


def _ragged_step(self, tokens):
    """standin_decode_shared.shared_step with the position row and the prefix length of every sequence's own group"""
    st = self.prefix
    lm = st.gpt.dist_model.language_model
    N, H, np_, hn, V, S, P, t, fan = self.batch, st.H, st.np_, st.hn, st.V, self.S, self.P, self.t, self.fan
    lens = self.group_prefix_len.tolist()
    assert P + t < lm.embedding.position_embeddings.weight.shape[0] and t < S and max(lens) <= P and min(lens) >= 1
    pos = torch.tensor(lens).repeat_interleave(fan) + t
    h = lm.embedding.word_embeddings.weight.float()[tokens.view(-1)] + lm.embedding.position_embeddings.weight.float()[pos]
    h = h.to(BF).view(N, H)
    cs = (S * 3 * H, 3 * hn, 3 * H)
    lay = so.AttnLayout(cs, cs, cs, (H, hn, H))
    ps = (P * 3 * H, 3 * hn, 3 * H)
    for li, layer in enumerate(lm.encoder.layers):
        att, mlp, pc, sc = layer.self_attention, layer.mlp, st.cache[li], self.suffix[li]
        x1, _, _ = so.layernorm_fwd(h, layer.input_layernorm.weight, layer.input_layernorm.bias, layer.input_layernorm.eps, N, H)
        so.gemm(x1, att.query_key_value.weight, N, 3 * H, H, bias=att.query_key_value.bias, cmap=(1, S, t), out=sc)
        ctx = attn_decode_shared_ragged_ref(sc[t:], sc[:, hn:], sc[:, 2 * hn:], pc[:, hn:], pc[:, 2 * hn:], lay, (ps, ps), N, fan, np_, lens,
                                            t + 1, hn, 1.0 / math.sqrt(hn)).to(BF).reshape(N, H)
        h1 = so.gemm(ctx, att.dense.weight, N, H, H, bias=att.dense.bias, residual=h)
        x2, _, _ = so.layernorm_fwd(h1, layer.post_attention_layernorm.weight, layer.post_attention_layernorm.bias,
                                    layer.post_attention_layernorm.eps, N, H)
        F4 = mlp.dense_h_to_4h.out_features
        g = so.gemm(x2, mlp.dense_h_to_4h.weight, N, F4, H, bias=mlp.dense_h_to_4h.bias, act=so.ACT_GELU_TANH)
        h = so.gemm(g, mlp.dense_4h_to_h.weight, N, H, F4, bias=mlp.dense_4h_to_h.bias, residual=h1)
    fl = lm.encoder.final_layernorm
    xf, _, _ = so.layernorm_fwd(h, fl.weight, fl.bias, fl.eps, N, H)
    return so.gemm(xf, lm.embedding.word_embeddings.weight, N, V, H)


def shared_step(self, tokens):
    """mpv_gpt_decode_step_shared(_ragged)(_q8) behind SharedPrefixDecodeState._shared_step: the uniform state goes to standin_w8's"""
    if self.group_prefix_len is None:
        return sw.shared_step(self, tokens)
    st = self.prefix
    real = st.gpt
    if st.q8 is not None:
        st.gpt = sw._dequantised_decoder(st.gpt, st.q8)
    try:
        return _ragged_step(self, tokens)
    finally:
        st.gpt = real


def _row_independent_products(monkeypatch):
    """The stand-ins multiply in fp32 through torch, whose BLAS picks a kernel -- and with it a summation order -- by the operand
    shapes: a row of a 25-row product may differ in its last bit from the same row of a 5-row product.  The mixed search runs other
    row counts than the grouped one it is compared with, and equal SCORES need bit-equal logits.  For the duration of a test every
    fp32 `@` therefore accumulates in fp64 and rounds once: a row's result no longer depends on its neighbours (the two orders
    differ by 1e-16 relative before a rounding to 24 bits)."""
    import torch.nn.functional as F

    def in_fp64(fn):
        def product(a, b, *rest, **kw):
            if torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == torch.float32 and b.dtype == torch.float32 and not rest and not kw:
                return fn(a.double(), b.double()).float()
            return fn(a, b, *rest, **kw)
        return product
    # every spelling of a product a stand-in could use, not only the `@` they use today (tests/test_decode_ragged_cpu.py checks them)
    for owner, name in ((torch.Tensor, "__matmul__"), (torch.Tensor, "matmul"), (torch.Tensor, "mm"), (torch.Tensor, "bmm"),
                        (torch, "matmul"), (torch, "mm"), (torch, "bmm"), (F, "linear")):
        monkeypatch.setattr(owner, name, in_fp64(getattr(owner, name)))


def install(monkeypatch):
    """standin_w8.install plus the ragged prefill, the ragged-aware step and products whose rows do not depend on the row count"""
    sw.install(monkeypatch)
    from youku_mplug_amd import generation
    monkeypatch.setattr(generation.SharedPrefixDecodeState, "_ragged_prefill", ragged_prefill)
    monkeypatch.setattr(generation.SharedPrefixDecodeState, "_shared_step", shared_step)
    _row_independent_products(monkeypatch)
