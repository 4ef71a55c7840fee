"""Torch stand-in for the shared-prefix attention (include/mpv.h: mpv_attn_prefix_fwd), TEST INFRASTRUCTURE ONLY, in the manner of
tests/standin_ops.py: it restates the C contract (query row i of continuation c at absolute position P + i sees the P prefix keys of
group c // group_size and its own keys j <= i; fp32 scores and softmax, bf16 probabilities into the PV product, bf16 output) with
plain torch on host tensors.  `install(monkeypatch)` installs standin_ops first and this on top."""
import torch

import standin_ops

BF = torch.bfloat16


def _view(t, st, a, heads, rows, hd):
    return t.as_strided((a, heads, rows, hd), (st[0], st[1], st[2], 1), t.storage_offset()).float()


def attn_prefix_fwd(q, k, v, pk, pv, o, lay, prefix_lay, n_cont, group_size, heads, cont_len, prefix_len, hd, *, scale=1.0):
    n_groups = (n_cont + group_size - 1) // group_size
    Lc, P = cont_len, prefix_len
    qf = _view(q, lay.q, n_cont, heads, Lc, hd)
    kf = _view(k, lay.k, n_cont, heads, Lc, hd)
    vf = _view(v, lay.v, n_cont, heads, Lc, hd)
    grp = torch.arange(n_cont) // group_size
    if P > 0:
        kp = _view(pk, prefix_lay[0], n_groups, heads, P, hd)[grp]
        vp = _view(pv, prefix_lay[1], n_groups, heads, P, hd)[grp]
        kf, vf = torch.cat([kp, kf], dim=2), torch.cat([vp, vf], dim=2)
    s = (qf @ kf.transpose(-1, -2)) * scale
    i, j = torch.arange(Lc)[:, None] + P, torch.arange(P + Lc)[None, :]
    s = s.masked_fill(j > i, float("-inf"))
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    o.as_strided((n_cont, heads, Lc, hd), (lay.o[0], lay.o[1], lay.o[2], 1), o.storage_offset()).copy_(
        ((standin_ops._r16(p) @ vf) / l).to(BF))
    return o


NAMES = ["attn_prefix_fwd"]


def install(monkeypatch):
    standin_ops.install(monkeypatch)
    from youku_mplug_amd import ops
    g = globals()
    for n in NAMES:
        monkeypatch.setattr(ops, n, g[n])
