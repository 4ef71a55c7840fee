"""The fp64 references of tests/ref_embed_glue.py are right, and a correct implementation fits inside the gates (no GPU).
First half: each reference against an implementation it shares nothing with -- F.unfold, F.embedding, autograd of a plain torch
forward (the backward kernels), torch.log_softmax + torch's stable sort, torch's own bf16 conversion, matrix products -- and the
rounding points the references add to those (bf16(pos + temporal), the bf16 cls mean and its two admissible roundings at a tie).
Second half: the torch stand-ins of tests/standin_ops.py over the cases of tests/test_embed_glue_kernels_gpu.py that are built on the
host (all but the nine past a grid cap), through the same runners and the SAME gates."""
import pytest
import torch
import torch.nn.functional as F

import embed_glue_cases as K
import ref_embed_glue as R
import standin_ops

BF = torch.bfloat16
F64 = torch.float64
CPU = torch.device("cpu")


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("B,C,T,H,W,P,kpad", [(2, 3, 2, 32, 48, 16, 768), (1, 3, 3, 28, 42, 14, 592), (2, 2, 1, 16, 8, 8, 136)])
def test_im2col_ref_matches_unfold(B, C, T, H, W, P, kpad):
    video = torch.randn(B, C, T, H, W, generator=_g(1)).to(BF)
    got = R.im2col_ref(video, B, C, T, H, W, P, kpad)
    want = F.unfold(video.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W).float(), P, stride=P).transpose(1, 2).reshape(-1, C * P * P)
    assert got.dtype == BF and torch.equal(got[:, :C * P * P].float(), want)
    assert K.same_bits(got[:, C * P * P:], torch.zeros_like(got[:, C * P * P:]))


def test_assemble_refs_match_a_plain_forward_and_its_autograd():
    """inputs of small integers: every sum is exact, bf16(pos + temporal) rounds nothing, and the forward is torch.cat of broadcasts;
    the backward reference is that forward's autograd"""
    B, T, N, D = 2, 3, 4, 8
    gen = _g(2)
    patch, cls, pos, tem = (torch.randint(-8, 9, s, generator=gen).to(F64).requires_grad_(True) for s in ((B * T * N, D), (D,), (N + 1, D), (T, D)))
    tok = patch.view(B, T, N, D) + pos[1:][None, None] + tem[None, :, None]
    x = torch.cat([(cls + pos[0]).expand(B, T, 1, D), tok], dim=2).reshape(-1, D)
    assert torch.equal(R.assemble_fwd_ref(patch.detach().to(BF), cls.detach().to(BF), pos.detach().to(BF), tem.detach().to(BF), B, T, N, D), x.detach())
    dx = torch.randn(B * T * (N + 1), D, generator=gen).to(BF)
    (x * dx.to(F64)).sum().backward()
    dpatch, (dpos, apos, npos), (dtem, atem, ntem) = R.assemble_bwd_ref(dx, B, T, N, D)
    assert torch.equal(dpatch.to(F64), patch.grad)
    assert (dpos - pos.grad).abs().max().item() <= 1e-13 and (dtem - tem.grad).abs().max().item() <= 1e-13
    assert (dpos[0] - cls.grad).abs().max().item() <= 1e-13
    assert (npos, ntem) == (B * T, B * N) and bool((apos >= dpos.abs()).all()) and bool((atem >= dtem.abs()).all())


def test_assemble_fwd_ref_rounds_pos_plus_temporal_to_bf16_first():
    one = lambda v: torch.tensor([[v] * 4], dtype=BF)
    x = R.assemble_fwd_ref(one(2.0 ** -8), one(0.5)[0], torch.tensor([[1.0] * 4] * 2, dtype=BF), one(2.0 ** -8), 1, 1, 1, 4)
    # cls row: 0.5 + 1 (no temporal term); token: 2^-8 + bf16(1 + 2^-8) = 2^-8 + 1, not 1 + 2^-7
    assert x.tolist() == [[1.5] * 4, [1.0 + 2.0 ** -8] * 4]


def test_cls_merge_refs_match_a_plain_forward_and_its_autograd():
    """T = 4 and integer inputs: the mean is a multiple of 1/4, exact in bf16, so the reference is the plain forward; its backward is
    that forward's autograd"""
    B, T, N1, D = 2, 4, 3, 4
    gen = _g(3)
    xt = torch.randint(-8, 9, (B * T * N1, D), generator=gen).to(F64)
    a = torch.randint(-8, 9, (B * T * N1, D), generator=gen).to(F64).requires_grad_(True)
    av = a.view(B, T, N1, D)
    y = xt.view(B, T, N1, D) + torch.cat([av[:, :, :1].mean(1, keepdim=True).expand(B, T, 1, D), av[:, :, 1:]], dim=2)
    ry, ry_alt = R.cls_merge_fwd_ref(xt.to(BF), a.detach().to(BF), B, T, N1, D)
    assert torch.equal(ry, y.detach().reshape(-1, D)) and torch.equal(ry_alt, ry)
    dy = torch.randn(B * T * N1, D, generator=gen).to(BF)
    (y.reshape(-1, D) * dy.to(F64)).sum().backward()
    mean, amean, n = R.cls_merge_bwd_ref(dy, B, T, N1, D)
    g = a.grad.view(B, T, N1, D)
    assert torch.equal(g[:, :, 1:], dy.to(F64).view(B, T, N1, D)[:, :, 1:])
    assert (g[:, :, 0] - mean[:, None]).abs().max().item() <= 1e-15 and n == T + 2 and bool((amean >= mean.abs()).all())


def test_r16_both_offers_the_other_rounding_only_at_a_tie():
    x = torch.tensor([1.0 + 2.0 ** -8 + 1e-9, 1.0 + 2.0 ** -8 - 1e-9, 1.0 + 2.0 ** -9, -(1.0 + 3 * 2.0 ** -8) + 1e-9, 3.0], dtype=F64)
    m, alt = R.r16_both(x, torch.full_like(x, 1e-8))
    assert m.tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0, -(1.0 + 2.0 ** -7), 3.0]
    assert alt.tolist() == [1.0, 1.0 + 2.0 ** -7, 1.0, -(1.0 + 2.0 ** -6), 3.0]
    up, down = R.bf16_step(torch.tensor([1.0, -1.0, 2.0], dtype=F64), torch.tensor([True, True, False]))[0:2], None
    assert up.tolist() == [1.0 + 2.0 ** -7, -(1.0 - 2.0 ** -8)]
    assert R.bf16_step(torch.tensor([2.0], dtype=F64), torch.tensor([False])).tolist() == [2.0 - 2.0 ** -7]


def test_colsum_and_add_refs():
    x = torch.randn(700, 12, generator=_g(4)).to(BF)
    out0 = torch.randn(12, generator=_g(5)).to(BF)
    s, sa, n = R.colsum_ref(x, out0)
    assert (s - (x.double().sum(0) + out0.double())).abs().max().item() <= 1e-11 and n == 701
    assert (sa - (x.double().abs().sum(0) + out0.double().abs())).abs().max().item() <= 1e-11
    s2, _, n2 = R.colsum_ref(x)
    assert (s2 - x.double().sum(0)).abs().max().item() <= 1e-11 and n2 == 700
    assert torch.equal(R.add_ref(x, x), 2 * x.double())


def test_gpt_embed_refs_match_embedding_lookups_and_autograd():
    B, Q, L, H, V = 2, 3, 4, 8, 20
    gen = _g(6)
    query, wte, wpe = (torch.randn(s, generator=gen).to(BF) for s in ((B * Q, H), (V, H), (Q + L, H)))
    ids = torch.randint(0, V, (B, L), generator=gen)
    h = (torch.cat([query.double().view(B, Q, H), F.embedding(ids, wte.double())], dim=1) + wpe.double()[None]).requires_grad_(True)
    assert torch.equal(R.gpt_embed_fwd_ref(query, ids, wte, wpe, B, Q, L, H), h.detach().view(-1, H))
    keep = R.keep_mask(K.DROP_SEED, K.DROP_OFFSET, B * (Q + L), H, 0.5)
    scale = R.drop_scale(0.5)
    dropped = R.gpt_embed_fwd_ref(query, ids, wte, wpe, B, Q, L, H, keep, scale)
    assert torch.equal(dropped, h.detach().view(-1, H).to(BF).double() * keep.double() * scale)
    dh = torch.randn(B * (Q + L), H, generator=gen).to(BF)
    ((h.view(-1, H) * keep.double() * scale) * dh.double()).sum().backward()
    assert torch.equal(R.gpt_embed_bwd_full_ref(dh, keep, scale), h.grad.view(-1, H))
    assert torch.equal(R.gpt_embed_bwd_full_ref(dh), dh.double())
    pos = [-4, 0, 6, 7, 100]
    idr = torch.randint(0, V, (5,), generator=gen)
    want = F.embedding(idr, wte.double()) + F.embedding(torch.tensor(pos).clamp(0, Q + L - 1), wpe.double())
    assert torch.equal(R.gpt_embed_rows_ref(idr, pos, wte, wpe), want)


@pytest.mark.parametrize("V,k", [(8, 8), (33, 5), (1000, 64)])
def test_logprob_topk_ref_matches_log_softmax_and_stable_sort(V, k):
    x = K.topk_rows(V, k, _g(7))
    add = torch.tensor(K.TOPK_ADDS * len(K.TOPK_KINDS), dtype=torch.float32)
    val, idx, lse = R.logprob_topk_ref(x, k, add)
    order = torch.sort(x.float(), dim=1, descending=True, stable=True).indices[:, :k]
    assert torch.equal(idx, order)
    lp = torch.log_softmax(x.double(), dim=1).gather(1, order) + add.double()[:, None]
    fin = torch.isfinite(lp)
    assert torch.equal(val[~fin], lp[~fin]) and ((val[fin] - lp[fin]).abs() <= 1e-12 * lp[fin].abs() + 1e-12).all()
    assert (lse - torch.logsumexp(x.double(), dim=1)).abs().max().item() <= 1e-12
    val0, idx0, _ = R.logprob_topk_ref(x, k)
    assert torch.equal(idx0, idx) and torch.isfinite(val0).all()
    assert float(K.topk_atol(lse, add).min()) >= K.GATES["topk.values"][1] and float(K.topk_atol(lse, None).max()) <= K.TOPK_ATOL_CAP


def test_ban_is_generations_ban_beam():
    from youku_mplug_amd import generation
    assert K.BAN == generation.BAN_BEAM == torch.tensor(generation.BAN_BEAM).to(BF).item()


def test_f32_to_bf16_ref_matches_torch_and_the_listed_roundings():
    src = torch.cat([torch.tensor(K.F32_SPECIALS, dtype=torch.float32), torch.randn(4096, generator=_g(8)) * 1e3, torch.randn(4096, generator=_g(9)) * 1e-39])
    assert K.same_bits(R.f32_to_bf16_ref(src), src.to(BF))
    got = R.f32_to_bf16_ref(torch.tensor(K.F32_SPECIALS[:7], dtype=torch.float32)).tolist()
    assert got == [1.0, 1.0 + 2.0 ** -6, -1.0, 1.0 + 2.0 ** -7, 2.0, 2.0, float("inf")]
    gs = [torch.tensor([1.0, 2.0 ** -24], dtype=BF), torch.tensor([2.0 ** -30, 1.0], dtype=BF), torch.tensor([1.0, 1.0], dtype=BF)]
    assert R.accum_f32_ref(gs).tolist() == [2.0, 2.0]      # fp32, in call order: 1 + 2^-30 rounds to 1; 2^-24 + 1 is a tie and goes to the even 1


def test_compose_refs_match_matrix_products():
    D = 24
    gen = _g(10)
    P, wf = torch.randn(D, D, generator=gen).to(BF), torch.randn(D, D, generator=gen).to(BF)
    dbc, bp, bfv = (torch.randn(D, generator=gen).to(BF) for _ in range(3))
    dwf, (dbp, adbp, n) = R.compose_finish_ref(P, dbc, bp, wf, D)
    assert (dwf - (P.double() + torch.outer(dbc.double(), bp.double()))).abs().max().item() <= 1e-13
    assert (dbp - wf.double().t() @ dbc.double()).abs().max().item() <= 1e-12 and n == D
    assert (adbp - wf.double().abs().t() @ dbc.double().abs()).abs().max().item() <= 1e-12
    bc, abc, n = R.compose_bias_ref(wf, bp, bfv, D)
    assert (bc - (wf.double() @ bp.double() + bfv.double())).abs().max().item() <= 1e-12 and n == D + 1
    assert (abc - (wf.double().abs() @ bp.double().abs() + bfv.double().abs())).abs().max().item() <= 1e-12


@pytest.mark.parametrize("with_plen", [False, True])
def test_caption_targets_ref_matches_the_tensor_expression(with_plen):
    B, L = 4, 9
    gen = _g(11)
    ids = torch.randint(0, 1000, (B, L), generator=gen)
    mask = (torch.arange(L)[None] < torch.tensor([9, 3, 0, 6])[:, None]).long()
    pl = torch.tensor([0, 1, 2, 8]) if with_plen else None
    labels, w = R.caption_targets_ref(ids, mask, pl)
    tla = mask[:, 1:].clone()
    if with_plen:
        tla[torch.arange(L - 1)[None] < pl.view(-1, 1)] = 0
    want = torch.zeros(B, L, dtype=F64)
    want[:, :L - 1] = tla.double() / tla.double().sum()
    assert torch.equal(labels.view(B, L), torch.cat([ids[:, 1:], ids[:, 1:2]], dim=1))
    assert (w.view(B, L) - want).abs().max().item() <= 1e-16
    l1, w1 = R.caption_targets_ref(ids[:, :1], mask[:, :1])
    assert not l1.any() and not w1.any()


def test_gates_are_the_derived_numbers():
    assert K.GATES["one_op"] == (2.0 ** -8 + 2.0 ** -23, 0.0) and K.GATES["sum"] == (2.0 ** -8, 1.0)
    assert K.GATES["caption.weights"] == (2.0 ** -23, 0.0)
    rtol, atol = K.GATES["topk.values"]
    assert rtol == 2.0 ** -22 and atol == 1.4e-6 and K.TOPK_ATOL_CAP == 1.4e-5      # the CE gate; topk_atol widens it per row, tenfold at most
    assert K.DROP_OFFSET % 2 == 0 and K.DROP_OFFSET % 8 != 0 and K.DROP_SEED >> 32


# ------------------------------------------------------------------------------------------------------------------ stand-ins
@pytest.fixture(autouse=True)
def _strict_standin(monkeypatch):
    """the assembly stand-in in the kernel's documented order (standin_ops.EMBED_STRICT): bf16(pos + temporal) before the token is added"""
    monkeypatch.setattr(standin_ops, "EMBED_STRICT", True)


@pytest.mark.parametrize("name,entry,args,kw", K.HOST_RUNS, ids=[r[0] for r in K.HOST_RUNS])
def test_standin_fits_the_gates(name, entry, args, kw):
    """every case of the device suite that is built on the host, through the same runner and gates, on the torch stand-in of the entry
    point.  The cases past a grid cap (embed_glue_cases.WRAP_RUNS: tens of MB each, built on the device) are about the kernels' stride
    loops, which a stand-in does not have: they run in the device file only, as the LayerNorm suite's wrap case does."""
    K.TABLES[entry][0](standin_ops, CPU, *args, **kw)
