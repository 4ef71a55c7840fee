"""Torch stand-ins for the two training entries of the packed shared-prefix attention (include/mpv.h: mpv_attn_prefix_packed_fwd_lse,
mpv_attn_prefix_packed_bwd), TEST INFRASTRUCTURE ONLY, in the manner of tests/standin_prefix_packed.py: the C contracts restated with
plain fp32 torch on host tensors -- P = exp(scale s - lse), delta from the bf16 o given, dS and P rounded to bf16 before their products,
bf16 outputs, a group's dpk / dpv summed in fp32 and rounded once (on top of what is there with accumulate_prefix).
`install(monkeypatch)` installs standin_prefix_packed first and this on top."""
import torch

import standin_ops
import standin_prefix
import standin_prefix_packed
from standin_prefix_packed import _rows

BF = torch.bfloat16


def _gview(t, st, G, heads, P, hd):
    return t.as_strided((G, heads, P, hd), (st[0], st[1], st[2], 1), t.storage_offset())


def _conts(layout):
    seg, grp = layout.seg_start.tolist(), layout.group_row.tolist()
    out, r = [], 0
    while r < layout.rows:
        e = r
        while e < layout.rows and seg[e] == r:
            e += 1
        out.append((max(g for g in range(layout.n_groups) if grp[g] <= r), r, e - r))
        r = e
    return out


def _keys(kf, vf, kp, vp, g, a, n, P):
    kk, vv = kf[a:a + n].transpose(0, 1), vf[a:a + n].transpose(0, 1)                    # [heads, n, hd]
    if P > 0:
        kk, vv = torch.cat([kp[g], kk], dim=1), torch.cat([vp[g], vv], dim=1)
    i, j = torch.arange(n)[:, None], torch.arange(P + n)[None, :]
    return kk, vv, (j < P) | (j - P <= i)


def attn_prefix_packed_fwd_lse(q, k, v, pk, pv, o, row_strides, prefix_lay, layout, heads, prefix_len, hd, *, scale=1.0, lse=None):
    R, P = layout.rows, prefix_len
    qf, kf, vf = (_rows(t, st, R, heads, hd).float() for t, st in zip((q, k, v), row_strides[:3]))
    of = _rows(o, row_strides[3], R, heads, hd)
    lse = torch.empty((heads, R), dtype=torch.float32) if lse is None else lse
    kp = vp = None
    if P > 0:
        kp = standin_prefix._view(pk, prefix_lay[0], layout.n_groups, heads, P, hd)
        vp = standin_prefix._view(pv, prefix_lay[1], layout.n_groups, heads, P, hd)
    for g, a, n in _conts(layout):
        kk, vv, vis = _keys(kf, vf, kp, vp, g, a, n, P)
        s = (torch.einsum("nhd,hkd->hnk", qf[a:a + n], kk) * scale).masked_fill(~vis, float("-inf"))
        m = s.max(-1, keepdim=True).values
        p = torch.exp(s - m)
        l = p.sum(-1, keepdim=True)
        of[a:a + n] = (torch.einsum("hnk,hkd->nhd", standin_ops._r16(p), vv) / l.transpose(0, 1)).to(BF)
        lse[:, a:a + n] = (m + torch.log(l))[..., 0]
    return lse


def attn_prefix_packed_bwd(q, k, v, pk, pv, o, lse, do, dq, dk, dv, dpk, dpv, row_strides, prefix_lay, layout, heads, prefix_len, hd, *,
                           scale=1.0, accumulate_prefix=False):
    R, P, G = layout.rows, prefix_len, layout.n_groups
    qf, kf, vf = (_rows(t, st, R, heads, hd).float() for t, st in zip((q, k, v), row_strides[:3]))
    of, dof = (_rows(t, row_strides[3], R, heads, hd).float() for t in (o, do))
    dqv, dkv, dvv = (_rows(t, st, R, heads, hd) for t, st in zip((dq, dk, dv), row_strides[:3]))
    kp = vp = None
    if P > 0:
        kp = standin_prefix._view(pk, prefix_lay[0], G, heads, P, hd)
        vp = standin_prefix._view(pv, prefix_lay[1], G, heads, P, hd)
        dkp, dvp = _gview(dpk, prefix_lay[0], G, heads, P, hd), _gview(dpv, prefix_lay[1], G, heads, P, hd)
        sum_k = dkp.float() if accumulate_prefix else torch.zeros(G, heads, P, hd)
        sum_v = dvp.float() if accumulate_prefix else torch.zeros(G, heads, P, hd)
    for g, a, n in _conts(layout):
        kk, vv, vis = _keys(kf, vf, kp, vp, g, a, n, P)
        s = torch.einsum("nhd,hkd->hnk", qf[a:a + n], kk) * scale
        p = torch.where(vis, torch.exp(s - lse[:, a:a + n, None]), torch.zeros(()))
        delta = (dof[a:a + n] * of[a:a + n]).sum(-1).transpose(0, 1)                      # [heads, n]
        ds = standin_ops._r16(p * (torch.einsum("nhd,hkd->hnk", dof[a:a + n], vv) - delta[..., None]))
        dqv[a:a + n] = (torch.einsum("hnk,hkd->nhd", ds, kk) * scale).to(BF)
        dk_all = torch.einsum("hnk,nhd->hkd", ds, qf[a:a + n]) * scale
        dv_all = torch.einsum("hnk,nhd->hkd", standin_ops._r16(p), dof[a:a + n])
        dkv[a:a + n] = dk_all[:, P:].transpose(0, 1).to(BF)
        dvv[a:a + n] = dv_all[:, P:].transpose(0, 1).to(BF)
        if P > 0:
            sum_k[g] += dk_all[:, :P]
            sum_v[g] += dv_all[:, :P]
    if P > 0:
        dkp.copy_(sum_k.to(BF))
        dvp.copy_(sum_v.to(BF))


NAMES = ["attn_prefix_packed_fwd_lse", "attn_prefix_packed_bwd"]


def install(monkeypatch):
    standin_prefix_packed.install(monkeypatch)
    from youku_mplug_amd import ops
    g = globals()
    for n in NAMES:
        monkeypatch.setattr(ops, n, g[n])
