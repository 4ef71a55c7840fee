"""Torch stand-ins of the shared-prefix decode path (include/mpv.h: mpv_attn_decode_shared_fwd, mpv_gpt_decode_step_shared) on
host tensors: the attention (one fp32 softmax over the group's prefix keys followed by the sequence's own keys, which is also the
reference of the kernel's GPU test, and its element-by-element fp64 definition) and the decode step behind
generation.SharedPrefixDecodeState, composed from tests/standin_ops.py.  install() adds them to the stand-ins of that module."""
import math

import torch

import standin_ops as so

BF = torch.bfloat16


def _view(t, st, n, heads, rows, hd):
    return t.as_strided((n, heads, rows, hd), (st[0], st[1], st[2], 1), t.storage_offset())


def attn_decode_shared_ref(q, k, v, pk, pv, lay, prefix_lay, n_seq, group_size, heads, prefix_len, own_len, hd, scale):
    """fp32 torch: one softmax over the group's prefix keys followed by the sequence's own keys, from the bf16 operands, nothing
    rounded on the way -> [n_seq, heads, hd] fp32.  The reference of the GPU kernel test; reads nothing at or beyond own_len."""
    n_groups = (n_seq + group_size - 1) // group_size
    qf = _view(q, (lay.q[0], lay.q[1], 0), n_seq, heads, 1, hd).float()
    kf = _view(k, lay.k, n_seq, heads, own_len, hd).float()
    vf = _view(v, lay.v, n_seq, heads, own_len, hd).float()
    grp = torch.arange(n_seq, device=q.device) // group_size
    pkf = _view(pk, prefix_lay[0], n_groups, heads, prefix_len, hd).float()[grp]
    pvf = _view(pv, prefix_lay[1], n_groups, heads, prefix_len, hd).float()[grp]
    keys, vals = torch.cat((pkf, kf), dim=2), torch.cat((pvf, vf), dim=2)
    s = (qf @ keys.transpose(-1, -2)) * scale
    return (torch.softmax(s, dim=-1) @ vals)[:, :, 0]


def attn_decode_shared_fwd(q, k, v, pk, pv, o, lay, prefix_lay, n_seq, group_size, heads, prefix_len, own_len, hd, *, scale=1.0):
    """ops.attn_decode_shared_fwd: refuses what the library refuses (ValueError here), o in bf16"""
    if hd not in (64, 80) or group_size < 1 or prefix_len < 1 or not 1 <= own_len <= 2048 or n_seq < 1 or heads < 1:
        raise ValueError("mpv_attn_decode_shared_fwd: unsupported shape")
    out = attn_decode_shared_ref(q, k, v, pk, pv, lay, prefix_lay, n_seq, group_size, heads, prefix_len, own_len, hd, scale)
    _view(o, (lay.o[0], lay.o[1], 0), n_seq, heads, 1, hd).copy_(out[:, :, None].to(BF))
    return o


def reference_fp64(q, k, v, pk, pv, lay, prefix_lay, n_seq, group_size, heads, prefix_len, own_len, hd, scale):
    """the definition, element by element in fp64: for sequence s and head h, softmax(scale * K q) V over K / V = the prefix rows of
    group s // group_size followed by the sequence's own rows -> [n_seq, heads, hd] fp64"""
    def row(t, base):
        return t.reshape(-1)[base:base + hd].double()
    (pks, pkh, pkr), (pvs, pvh, pvr) = prefix_lay
    out = torch.empty((n_seq, heads, hd), dtype=torch.float64)
    for s in range(n_seq):
        g = s // group_size
        for h in range(heads):
            qv = row(q, s * lay.q[0] + h * lay.q[1])
            K = torch.stack([row(pk, g * pks + h * pkh + j * pkr) for j in range(prefix_len)] +
                            [row(k, s * lay.k[0] + h * lay.k[1] + j * lay.k[2]) for j in range(own_len)])
            V = torch.stack([row(pv, g * pvs + h * pvh + j * pvr) for j in range(prefix_len)] +
                            [row(v, s * lay.v[0] + h * lay.v[1] + j * lay.v[2]) for j in range(own_len)])
            out[s, h] = torch.softmax((K @ qv) * scale, dim=0) @ V
    return out


def make_case(hd, heads, groups, group_size, prefix_len, own_len, short_last=0, suffix_max=None, seed=0, device="cpu", pad=0.0):
    """Operands laid out as the real caches are: prefix cache [groups * prefix_len, 3H] and suffix cache [n_seq * suffix_max, 3H]
    with head-interleaved q|k|v rows (H = heads * hd); the query of a sequence is the q third of its suffix row own_len - 1.  Suffix
    rows at and beyond own_len are filled with `pad`.  -> dict(args for attn_decode_shared_fwd, o, n_seq)."""
    H = heads * hd
    n_seq = groups * group_size - short_last
    S = suffix_max or own_len + 2
    g = torch.Generator().manual_seed(seed)
    prefix = torch.randn(groups * prefix_len, 3 * H, generator=g).to(BF)
    suffix = torch.randn(n_seq, S, 3 * H, generator=g).to(BF)
    suffix[:, own_len:] = pad
    suffix = suffix.view(n_seq * S, 3 * H)
    prefix, suffix = prefix.to(device), suffix.to(device)
    o = torch.zeros(n_seq, H, dtype=BF, device=device)
    cs = (S * 3 * H, 3 * hd, 3 * H)
    lay = so.AttnLayout(cs, cs, cs, (H, hd, H))
    ps = (prefix_len * 3 * H, 3 * hd, 3 * H)
    qv = suffix.view(-1)[(own_len - 1) * 3 * H:]
    kv, vv = suffix.view(-1)[hd:], suffix.view(-1)[2 * hd:]
    pkv, pvv = prefix.view(-1)[hd:], prefix.view(-1)[2 * hd:]
    return dict(q=qv, k=kv, v=vv, pk=pkv, pv=pvv, o=o, lay=lay, prefix_lay=(ps, ps), n_seq=n_seq, group_size=group_size, heads=heads,
                prefix_len=prefix_len, own_len=own_len, hd=hd, scale=1.0 / math.sqrt(hd), prefix=prefix, suffix=suffix, S=S)


def run_case(fn, c):
    return fn(c["q"], c["k"], c["v"], c["pk"], c["pv"], c["o"], c["lay"], c["prefix_lay"], c["n_seq"], c["group_size"], c["heads"],
              c["prefix_len"], c["own_len"], c["hd"], scale=c["scale"])


# (hd, heads, groups, group_size, prefix_len, own_len, short_last): every value of the issue's lists at least once, and the tile
# edges -- 32 / 33 rows, 31 / 32 / 33 and 64 / 65 prefix keys (one 32-key tile, a chunk of four is 128), own_len 1, own_len 33 (two
# own tiles per row) and 70 (three), a short last group, more than one chunk of own tiles (8 x 1, 32 x 1, 5 x 3 tiles).
SWEEP = [
    (64, 1, 1, 1, 1, 1, 0),
    (64, 3, 3, 5, 264, 2, 0),
    (80, 3, 1, 5, 31, 33, 0),
    (64, 1, 3, 8, 32, 1, 0),
    (80, 1, 3, 32, 33, 2, 0),
    (64, 3, 1, 33, 64, 1, 0),
    (80, 1, 1, 33, 65, 33, 0),
    (64, 1, 3, 5, 65, 70, 2),
    (80, 3, 3, 8, 264, 70, 5),
    (64, 1, 1, 32, 264, 33, 0),
]


def shared_step(self, tokens):
    """mpv_gpt_decode_step_shared behind generation.SharedPrefixDecodeState._shared_step, composed from the stand-ins"""
    st = self.prefix
    gpt = st.gpt
    lm = gpt.dist_model.language_model
    N, H, np_, hn, V, S, P, t = self.batch, st.H, st.np_, st.hn, st.V, self.S, self.P, self.t
    assert P + t < lm.embedding.position_embeddings.weight.shape[0] and t < S
    h = lm.embedding.word_embeddings.weight.float()[tokens.view(-1)] + lm.embedding.position_embeddings.weight.float()[P + t][None]
    h = h.to(BF).view(N, H)
    cs = (S * 3 * H, 3 * hn, 3 * H)
    lay = so.AttnLayout(cs, cs, cs, (H, hn, H))
    ps = (P * 3 * H, 3 * hn, 3 * H)
    for li, layer in enumerate(lm.encoder.layers):
        att, mlp, pc, sc = layer.self_attention, layer.mlp, st.cache[li], self.suffix[li]
        x1, _, _ = so.layernorm_fwd(h, layer.input_layernorm.weight, layer.input_layernorm.bias, layer.input_layernorm.eps, N, H)
        so.gemm(x1, att.query_key_value.weight, N, 3 * H, H, bias=att.query_key_value.bias, cmap=(1, S, t), out=sc)
        ctx = torch.zeros((N, H), dtype=BF)
        attn_decode_shared_fwd(sc[t:], sc[:, hn:], sc[:, 2 * hn:], pc[:, hn:], pc[:, 2 * hn:], ctx, lay, (ps, ps), N, self.fan, np_, P, t + 1, hn,
                               scale=1.0 / math.sqrt(hn))
        h1 = so.gemm(ctx, att.dense.weight, N, H, H, bias=att.dense.bias, residual=h)
        x2, _, _ = so.layernorm_fwd(h1, layer.post_attention_layernorm.weight, layer.post_attention_layernorm.bias,
                                    layer.post_attention_layernorm.eps, N, H)
        F4 = mlp.dense_h_to_4h.out_features
        g = so.gemm(x2, mlp.dense_h_to_4h.weight, N, F4, H, bias=mlp.dense_h_to_4h.bias, act=so.ACT_GELU_TANH)
        h = so.gemm(g, mlp.dense_4h_to_h.weight, N, H, F4, bias=mlp.dense_4h_to_h.bias, residual=h1)
    fl = lm.encoder.final_layernorm
    xf, _, _ = so.layernorm_fwd(h, fl.weight, fl.bias, fl.eps, N, H)
    return so.gemm(xf, lm.embedding.word_embeddings.weight, N, V, H)


def install(monkeypatch):
    """standin_ops.install plus the shared-prefix attention and step"""
    so.install(monkeypatch)
    from youku_mplug_amd import generation, ops
    monkeypatch.setattr(ops, "attn_decode_shared_fwd", attn_decode_shared_fwd)
    monkeypatch.setattr(generation.SharedPrefixDecodeState, "_shared_step", shared_step)
