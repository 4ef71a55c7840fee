"""mpv_attn_prefix_fwd (csrc/prefix_attention.hip): causal attention of continuations against a shared prefix, against an fp32
torch reference built on the materialised concatenation [prefix K/V | own K/V], and against the decoder's own mpv_attn_fwd on that
same concatenation (the kernel it stands in for must not be beaten by more than 1.5x in error)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _problem(dev, hd, heads, G, P, Lc, n_groups, seed, short_last=0):
    """packed qkv rows as the decoder's qkv product writes them: [rows, 3H], head h at columns h*3hn (q), +hn (k), +2hn (v)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    H = heads * hd
    n_cont = n_groups * G - short_last
    cq = (torch.randn(n_cont * Lc, 3 * H, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    pq = (torch.randn(n_groups * P, 3 * H, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    return cq, pq, n_cont, H


def _run_prefix(cq, pq, n_cont, G, P, Lc, heads, hd):
    from youku_mplug_amd import ops
    H = heads * hd
    o = torch.empty((n_cont * Lc, H), dtype=torch.bfloat16, device=cq.device)
    st3 = (Lc * 3 * H, 3 * hd, 3 * H)
    lay = ops.AttnLayout(st3, st3, st3, (Lc * H, hd, H))
    pst = (P * 3 * H, 3 * hd, 3 * H)
    ops.attn_prefix_fwd(cq, cq[:, hd:], cq[:, 2 * hd:], pq[:, hd:], pq[:, 2 * hd:], o, lay, (pst, pst), n_cont, G, heads, Lc, P, hd,
                        scale=1.0 / math.sqrt(hd))
    torch.cuda.synchronize()
    return o


def _concat(cq, pq, n_cont, G, P, Lc, H):
    """[n_cont, P + Lc, 3H]: every continuation behind a copy of its group's prefix rows"""
    if P == 0:
        return cq.view(n_cont, Lc, 3 * H).contiguous()
    grp = torch.arange(n_cont, device=cq.device) // G
    pre = pq.view(-1, P, 3 * H)[grp]
    return torch.cat([pre, cq.view(n_cont, Lc, 3 * H)], dim=1).contiguous()


def _ref_fp32(full, n_cont, P, Lc, heads, hd):
    S = P + Lc
    x = full.float().view(n_cont, S, heads, 3, hd)
    q, k, v = x[..., 0, :], x[..., 1, :], x[..., 2, :]
    s = torch.einsum("bihd,bjhd->bhij", q[:, P:], k) / math.sqrt(hd)
    i = torch.arange(Lc, device=full.device)[:, None] + P
    j = torch.arange(S, device=full.device)[None, :]
    s = s.masked_fill(j > i, float("-inf"))
    o = torch.einsum("bhij,bjhd->bihd", torch.softmax(s, dim=-1), v)
    return o.reshape(n_cont * Lc, heads * hd)


def _existing_kernel(full, n_cont, P, Lc, heads, hd):
    from youku_mplug_amd import ops
    S, H = P + Lc, heads * hd
    o = torch.empty((n_cont * S, H), dtype=torch.bfloat16, device=full.device)
    st3 = (S * 3 * H, 3 * hd, 3 * H)
    fl = full.view(n_cont * S, 3 * H)
    ops.attn_fwd(fl, fl[:, hd:], fl[:, 2 * hd:], o, ops.AttnLayout(st3, st3, st3, (S * H, hd, H)), n_cont, heads, S, S, hd, causal=True,
                 scale=1.0 / math.sqrt(hd))
    torch.cuda.synchronize()
    return o.view(n_cont, S, H)[:, P:].reshape(n_cont * Lc, H)


@pytest.mark.parametrize("hd", [64, 80])
def test_attn_prefix_fwd_sweep_vs_fp32_and_the_decoder_kernel(dev, hd):
    heads, n_groups = 2, 3
    worst = []
    for G in (1, 8, 45):
        for P in (0, 1, 128, 137, 213):               # (0: no prefix, phase 1 skipped)
            for Lc in (1, 5, 33, 80):
                short = 1 if G > 1 else 0            # the last group one continuation short
                cq, pq, n_cont, H = _problem(dev, hd, heads, G, P, Lc, n_groups, seed=hd * 1000 + G * 97 + P * 7 + Lc, short_last=short)
                mine = _run_prefix(cq, pq, n_cont, G, P, Lc, heads, hd).float()
                full = _concat(cq, pq, n_cont, G, P, Lc, H)
                ref = _ref_fp32(full, n_cont, P, Lc, heads, hd)
                base = _existing_kernel(full, n_cont, P, Lc, heads, hd).float()
                assert torch.isfinite(mine).all(), (G, P, Lc)
                e_new = (mine - ref).abs().max().item()
                e_old = (base - ref).abs().max().item()
                worst.append((e_new / max(e_old, 1e-6), G, P, Lc, e_new, e_old))
                assert e_new <= 1.5 * e_old + 1e-6, (G, P, Lc, e_new, e_old)
    print("worst error ratio (new / mpv_attn_fwd):", max(worst))


@pytest.mark.parametrize("hd", [64, 80])
def test_attn_prefix_fwd_permutes_with_its_continuations(dev, hd):
    """Permuting continuations inside their groups, and permuting the groups (prefixes and their continuations together),
    permutes the output rows and changes nothing else."""
    heads, G, P, Lc, n_groups = 3, 8, 137, 33, 3
    cq, pq, n_cont, H = _problem(dev, hd, heads, G, P, Lc, n_groups, seed=5)
    out = _run_prefix(cq, pq, n_cont, G, P, Lc, heads, hd)
    gen = torch.Generator().manual_seed(11)
    gperm = torch.randperm(n_groups, generator=gen)
    cperm = torch.cat([gperm[g] * G + torch.randperm(G, generator=gen) for g in range(n_groups)])     # new continuation -> old
    cq2 = cq.view(n_cont, Lc, 3 * H)[cperm.to(dev)].reshape(n_cont * Lc, 3 * H).contiguous()
    pq2 = pq.view(n_groups, P, 3 * H)[gperm.to(dev)].reshape(n_groups * P, 3 * H).contiguous()
    out2 = _run_prefix(cq2, pq2, n_cont, G, P, Lc, heads, hd)
    want = out.view(n_cont, Lc, H)[cperm.to(dev)].reshape(n_cont * Lc, H)
    ref = _ref_fp32(_concat(cq, pq, n_cont, G, P, Lc, H), n_cont, P, Lc, heads, hd)
    tol = 2 * (out.float() - ref).abs().max().item()
    assert (out2.float() - want.float()).abs().max().item() <= tol


def test_attn_prefix_fwd_refuses_other_head_dims(dev):
    from youku_mplug_amd import _lib
    hd, heads, G, P, Lc = 96, 1, 2, 4, 3
    cq, pq, n_cont, H = _problem(dev, hd, heads, G, P, Lc, 1, seed=1)
    with pytest.raises(_lib.MpvError, match="head_dim 96"):
        _run_prefix(cq, pq, n_cont, G, P, Lc, heads, hd)
