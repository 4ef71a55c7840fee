"""Torch stand-ins for the two packed-row entry points (include/mpv.h: mpv_attn_prefix_packed_fwd, mpv_gpt_embed_rows_fwd), TEST
INFRASTRUCTURE ONLY, in the manner of tests/standin_prefix.py: they restate the C contracts with plain torch on host tensors (query row r
sees the prefix keys of its group and its own keys seg_start[r] <= kr <= r; fp32 scores and softmax, bf16 probabilities into the PV product,
bf16 output; out[r] = wte[ids[r]] + wpe[pos[r]] with one bf16 rounding).  `install(monkeypatch)` installs standin_prefix first and this on top."""
import torch

import standin_ops
import standin_prefix

BF = torch.bfloat16


def _rows(t, st, rows, heads, hd):
    return t.as_strided((rows, heads, hd), (st[0], st[1], 1), t.storage_offset())


def attn_prefix_packed_fwd(q, k, v, pk, pv, o, row_strides, prefix_lay, layout, heads, prefix_len, hd, *, scale=1.0):
    R, P = layout.rows, prefix_len
    seg, grp = layout.seg_start.tolist(), layout.group_row.tolist()
    assert len(seg) == R and grp[0] == 0 and grp[-1] == R and all(0 <= s <= r for r, s in enumerate(seg))
    qf, kf, vf = (_rows(t, st, R, heads, hd).float() for t, st in zip((q, k, v), row_strides[:3]))
    of = _rows(o, row_strides[3], R, heads, hd)
    for g in range(layout.n_groups):
        if P > 0:
            kp = standin_prefix._view(pk, prefix_lay[0], layout.n_groups, heads, P, hd)[g]       # [heads, P, hd]
            vp = standin_prefix._view(pv, prefix_lay[1], layout.n_groups, heads, P, hd)[g]
        for r in range(grp[g], grp[g + 1]):
            assert grp[g] <= seg[r], "a continuation never spans two groups"
            kk, vv = kf[seg[r]:r + 1].transpose(0, 1), vf[seg[r]:r + 1].transpose(0, 1)            # [heads, own, hd]
            if P > 0:
                kk, vv = torch.cat([kp, kk], dim=1), torch.cat([vp, vv], dim=1)
            s = torch.einsum("hd,hkd->hk", qf[r], kk) * scale
            p = torch.exp(s - s.max(-1, keepdim=True).values)
            of[r] = (torch.einsum("hk,hkd->hd", standin_ops._r16(p), vv) / p.sum(-1, keepdim=True)).to(BF)
    return o


def gpt_embed_rows_fwd(ids, pos, pos_host, wte, wpe, rows, H):
    from youku_mplug_amd import _lib
    if max(pos_host) >= wpe.shape[0]:                    # the wrapper's host-side refusal is part of the contract
        raise _lib.MpvError(f"sequence of {max(pos_host) + 1} positions exceeds max_position_embeddings = {wpe.shape[0]}")
    assert ids.numel() == rows and pos.tolist() == list(pos_host)
    return (wte.float()[ids.view(-1)] + wpe.float()[pos.view(-1).long()]).to(BF)


NAMES = ["attn_prefix_packed_fwd", "gpt_embed_rows_fwd"]


def install(monkeypatch):
    standin_prefix.install(monkeypatch)
    from youku_mplug_amd import ops
    g = globals()
    for n in NAMES:
        monkeypatch.setattr(ops, n, g[n])
