"""Scoring of given captions on the GPU: mpv_attn_prefix_packed_fwd (csrc/prefix_attention.hip) against an
fp32 torch softmax over every continuation's concatenated keys and against the decoder's own mpv_attn_fwd on that concatenation (the
gate of tests/test_prefix_attention_gpu.py), against mpv_attn_prefix_fwd at uniform lengths, and its bit-for-bit properties;
mpv_gpt_embed_rows_fwd against mpv_gpt_embed_fwd; DistributedGPT3_Caption.score_captions on the tiny model against three yardsticks; the
caption entry point's --eval_score_gold."""
import json
import math
import os

import pytest
import torch

import caption_score_cases as cs

gpu = pytest.mark.gpu
BF = torch.bfloat16
PREFIX_LENS = [0, 1, 31, 32, 33, 64, 65, 264]


def _problem(dev, hd, heads, lay, P, seed, extra_rows=0):
    """qkv rows as the decoder's qkv product writes them: [rows, 3H], head h at columns h*3hn (q), +hn (k), +2hn (v)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    H = heads * hd
    rows, ng = sum(lay[0]), len(lay[1])
    cq = (torch.randn(rows + extra_rows, 3 * H, generator=g) * 1.5).to(BF).to(dev)
    pq = (torch.randn(max(ng * P, 1), 3 * H, generator=g) * 1.5).to(BF).to(dev)
    return cq, pq, H


def _run_packed(cq, pq, layout, P, heads, hd, o=None, scale=None, hd_arg=None):
    from youku_mplug_amd import ops
    H = heads * hd
    o = torch.empty((layout.rows, H), dtype=BF, device=cq.device) if o is None else o
    st = ((3 * H, 3 * hd),) * 3 + ((H, hd),)
    pst = (P * 3 * H, 3 * hd, 3 * H)
    ops.attn_prefix_packed_fwd(cq, cq[:, hd:], cq[:, 2 * hd:], pq[:, hd:], pq[:, 2 * hd:], o, st, (pst, pst), layout, heads, P, hd_arg or hd,
                               scale=1.0 / math.sqrt(hd) if scale is None else scale)
    torch.cuda.synchronize()
    return o


def _references(cq, pq, lay, P, heads, hd):
    """(fp32 softmax over the concatenated keys of each continuation, mpv_attn_fwd causal on the materialised concatenation), both
    [rows, H] fp32 from the same bf16 operands; continuations of one length share a batch"""
    from youku_mplug_amd import ops
    dev, H = cq.device, heads * hd
    seg, grp, rows, _ = cs.layout_restated(*lay)
    ref = torch.empty((rows, H), dtype=torch.float32, device=dev)
    base = torch.empty((rows, H), dtype=torch.float32, device=dev)
    starts, groups, c = [], [], 0
    for g, n in enumerate(lay[1]):
        for _ in range(n):
            starts.append(sum(lay[0][:c]))
            groups.append(g)
            c += 1
    for n in sorted(set(lay[0])):
        idx = [c for c, ln in enumerate(lay[0]) if ln == n]
        own = torch.stack([cq[starts[c]:starts[c] + n] for c in idx])                              # [b, n, 3H]
        full = own if P == 0 else torch.cat([torch.stack([pq[groups[c] * P:(groups[c] + 1) * P] for c in idx]), own], dim=1)
        full = full.contiguous()
        b, S = len(idx), P + n
        x = full.float().view(b, S, heads, 3, hd)
        q, k, v = x[..., 0, :], x[..., 1, :], x[..., 2, :]
        s = torch.einsum("bihd,bjhd->bhij", q[:, P:], k) / math.sqrt(hd)
        i, j = torch.arange(n, device=dev)[:, None] + P, torch.arange(S, device=dev)[None, :]
        r = torch.einsum("bhij,bjhd->bihd", torch.softmax(s.masked_fill(j > i, float("-inf")), dim=-1), v).reshape(b, n, H)
        o = torch.empty((b * S, H), dtype=BF, device=dev)
        st3 = (S * 3 * H, 3 * hd, 3 * H)
        fl = full.view(b * S, 3 * H)
        ops.attn_fwd(fl, fl[:, hd:], fl[:, 2 * hd:], o, ops.AttnLayout(st3, st3, st3, (S * H, hd, H)), b, heads, S, S, hd, causal=True,
                     scale=1.0 / math.sqrt(hd))
        o = o.view(b, S, H)[:, P:].float()
        for t, c in enumerate(idx):
            ref[starts[c]:starts[c] + n] = r[t]
            base[starts[c]:starts[c] + n] = o[t]
    torch.cuda.synchronize()
    return ref, base


@gpu
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("hd", [64, 80])
def test_packed_attention_sweep_vs_fp32_and_the_decoder_kernel(dev, hd, heads):
    """e_new <= 1.5 * e_old + 1e-6 with e_old the error of mpv_attn_fwd (causal) on the materialised concatenation, in the same run"""
    from youku_mplug_amd import ops
    worst = []
    for li, lay in enumerate(cs.LAYOUTS):
        layout = ops.PackedLayout(*lay, device=dev)
        for P in PREFIX_LENS:
            cq, pq, H = _problem(dev, hd, heads, lay, P, seed=hd * 1000 + heads * 131 + li * 17 + P)
            mine = _run_packed(cq, pq, layout, P, heads, hd).float()
            ref, base = _references(cq, pq, lay, P, heads, hd)
            assert torch.isfinite(mine).all(), (lay, P)
            e_new, e_old = (mine - ref).abs().max().item(), (base - ref).abs().max().item()
            worst.append((e_new / max(e_old, 1e-6), cs.layout_id(lay), P, e_new, e_old))
            assert e_new <= 1.5 * e_old + 1e-6, (lay, P, e_new, e_old)
    print(f"    hd {hd} heads {heads}: {len(worst)} problems, worst error ratio (new / mpv_attn_fwd): {max(worst)}; largest e_new "
          f"{max(w[3] for w in worst):.3e}, largest e_old {max(w[4] for w in worst):.3e}")


@gpu
@pytest.mark.parametrize("hd", [64, 80])
def test_packed_attention_at_uniform_lengths_vs_the_uniform_kernel(dev, hd):
    """the same data through mpv_attn_prefix_fwd: both inside the gate above, their difference at most twice the older kernel's own error
    -- and in fact none: the two entries run one kernel body that cuts a group into the same tiles, so on a uniform layout they agree bit
    for bit.  (G, Lc, groups, P, continuations short in the last group): prefix phase skipped / a partial chunk / several chunks, the
    segment division on and off, a continuation across the 128-row tile edge (5 x 33 rows: the second tile's key stream starts inside
    the first), a short last group, workgroups that leave early."""
    from youku_mplug_amd import ops
    heads = 3
    for G, Lc, ng, P, short in ((8, 5, 3, 137, 0), (3, 41, 2, 264, 0), (45, 7, 2, 33, 0), (1, 130, 2, 0, 0), (8, 5, 3, 65, 1), (5, 33, 2, 31, 0)):
        n_cont = G * ng - short
        lay = ([Lc] * n_cont, [G] * (ng - 1) + [G - short])
        cq, pq, H = _problem(dev, hd, heads, lay, P, seed=hd + G * 7 + Lc)
        mine_bf = _run_packed(cq, pq, ops.PackedLayout(*lay, device=dev), P, heads, hd)
        mine = mine_bf.float()
        o = torch.empty((n_cont * Lc, H), dtype=BF, device=dev)
        st3 = (Lc * 3 * H, 3 * hd, 3 * H)
        pst = (P * 3 * H, 3 * hd, 3 * H)
        ops.attn_prefix_fwd(cq, cq[:, hd:], cq[:, 2 * hd:], pq[:, hd:], pq[:, 2 * hd:], o, ops.AttnLayout(st3, st3, st3, (Lc * H, hd, H)), (pst, pst),
                            n_cont, G, heads, Lc, P, hd, scale=1.0 / math.sqrt(hd))
        torch.cuda.synchronize()
        ref, base = _references(cq, pq, lay, P, heads, hd)
        e_new, e_uni, e_old = (mine - ref).abs().max().item(), (o.float() - ref).abs().max().item(), (base - ref).abs().max().item()
        diff = (mine - o.float()).abs().max().item()
        print(f"    hd {hd} G {G} Lc {Lc} P {P} n_cont {n_cont}: e_packed {e_new:.3e} e_uniform {e_uni:.3e} e_attn_fwd {e_old:.3e} "
              f"|packed - uniform| {diff:.3e}")
        assert e_new <= 1.5 * e_old + 1e-6 and e_uni <= 1.5 * e_old + 1e-6 and diff <= 2 * e_uni, (G, Lc, P, e_new, e_uni, e_old, diff)
        assert torch.equal(mine_bf, o), (G, Lc, P, n_cont, diff)


@gpu
@pytest.mark.parametrize("hd", [64, 80])
def test_a_continuation_depends_on_its_own_rows_and_its_groups_prefix_only(dev, hd):
    """overwriting q / k / v of every other continuation and every other group's prefix with different finite data leaves a continuation's
    output bits unchanged (a masked key is a true no-op); two runs are identical"""
    from youku_mplug_amd import ops
    heads, P = 3, 65
    for lay, targets in ((([33, 31, 32, 32, 5, 300], [3, 1, 2])), (0, 2, 3, 4, 5)), ((([7] * 19 + [3], [19, 1])), (0, 17, 18, 19)):
        layout = ops.PackedLayout(*lay, device=dev)
        cq, pq, H = _problem(dev, hd, heads, lay, P, seed=3 + hd)
        out = _run_packed(cq, pq, layout, P, heads, hd)
        assert torch.equal(out, _run_packed(cq, pq, layout, P, heads, hd))
        seg, grp, rows, _ = cs.layout_restated(*lay)
        starts = [sum(lay[0][:c]) for c in range(len(lay[0]))]
        g = torch.Generator().manual_seed(99)
        for t in targets:
            a, b = starts[t], starts[t] + lay[0][t]
            grp_t = max(i for i in range(len(lay[1])) if grp[i] <= a)
            cq2 = (torch.randn(cq.shape, generator=g) * 2.0).to(BF).to(dev)
            pq2 = (torch.randn(pq.shape, generator=g) * 2.0).to(BF).to(dev)
            cq2[a:b] = cq[a:b]
            pq2[grp_t * P:(grp_t + 1) * P] = pq[grp_t * P:(grp_t + 1) * P]
            out2 = _run_packed(cq2, pq2, layout, P, heads, hd)
            assert torch.equal(out2[a:b], out[a:b]), (lay, t)
            assert not torch.equal(out2, out)


@gpu
@pytest.mark.parametrize("hd", [64, 80])
def test_nothing_behind_the_rows_is_read_or_written_and_a_refusal_leaves_o_untouched(dev, hd):
    from youku_mplug_amd import _lib, ops
    heads, P, extra = 3, 33, 64
    lay = ([33, 31, 32, 32, 5], [3, 2])
    layout = ops.PackedLayout(*lay, device=dev)
    cq, pq, H = _problem(dev, hd, heads, lay, P, seed=8)
    want = _run_packed(cq, pq, layout, P, heads, hd)
    big = torch.full((layout.rows + extra, 3 * H), float("nan"), dtype=BF, device=dev)
    big[:layout.rows] = cq
    o = torch.full((layout.rows + extra, H), -7.0, dtype=BF, device=dev)
    _run_packed(big, pq, layout, P, heads, hd, o=o)
    assert torch.equal(o[:layout.rows], want) and torch.isfinite(o.float()).all() and (o[layout.rows:] == -7.0).all()
    o2 = torch.full((layout.rows, H), -7.0, dtype=BF, device=dev)
    for kw, msg in ((dict(scale=0.0), "scale"), (dict(hd_arg=96), "head_dim 96")):
        with pytest.raises(_lib.MpvError, match=msg):
            _run_packed(cq, pq, layout, P, heads, hd, o=o2, **kw)
    bad = ops.PackedLayout(*lay, device=dev)
    bad.max_group_rows = layout.rows + 1
    with pytest.raises(_lib.MpvError, match="max_group_rows"):
        _run_packed(cq, pq, bad, P, heads, hd, o=o2)
    torch.cuda.synchronize()
    assert (o2 == -7.0).all()


@gpu
@pytest.mark.parametrize("H", [160, 2048])
def test_embed_rows_equals_the_uniform_front_bit_for_bit(dev, H):
    from youku_mplug_amd import ops
    g = torch.Generator().manual_seed(H)
    V, S, P = 97, 40, 11
    wte = torch.randn(V, H, generator=g).to(BF).to(dev)
    wpe = torch.randn(S, H, generator=g).to(BF).to(dev)
    for B in (1, 3):
        for L in (1, 5):
            ids = torch.randint(0, V, (B, L), generator=g).to(dev)
            want = ops.gpt_embed_fwd(None, ids.contiguous(), wte, wpe[P:], B, 0, L, H)
            pos_host = [P + i for _ in range(B) for i in range(L)]
            pos = torch.tensor(pos_host, dtype=torch.int32, device=dev)
            got = ops.gpt_embed_rows_fwd(ids.view(-1).contiguous(), pos, pos_host, wte, wpe, B * L, H)
            torch.cuda.synchronize()
            assert got.shape == (B * L, H) and torch.equal(got, want), (B, L, H)


# ------------------------------------------------------------------------------ the tiny model
@gpu
def test_score_captions_against_three_yardsticks(dev):
    """All three compared with the fp32 restatement's teacher-forced log-probabilities of the same tokens (e_* = max abs deviation over the
    scored entries): (i) the padded forward_continuation on the same candidates, e_packed <= 1.5 * e_padded + 1e-6; (ii) the sampler's
    own scores of its samples (generate(do_sample=True, num_samples=4, return_scores=True), cut at the terminator), e_packed <= 1.5 *
    e_sampled + 1e-6 and the same counts; (iii) the golden anchor (tests/test_caption_score_cpu.py:golden_anchor) at PLAIN["caption_tiny"]
    ["score"] = 7e-3 relative."""
    from test_caption_score_cpu import golden_anchor
    from test_model_gpu import PLAIN
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    term = g["meta"]["eod_id"]
    vid = video.to(dev).to(BF)
    # (i)
    sel = [0, 1, 0, 1]
    cands = cs.ragged_candidates(cfg, [3] * 4, seed=33, avoid=term)
    text = cs.text_of(ids, mask, sel, dev)
    res = model.score_captions(vid[sel], text, cands, termination_id=term)
    qf = model.encode_video(vid[sel]).view(len(sel), -1, model.text_width)
    e_packed = e_padded = 0.0
    for pl, clips in ((5, [0, 2]), (3, [1, 3])):
        pad = cs.padded_logprobs(model, qf[clips].contiguous(), text.input_ids[clips], pl, [cands[i] for i in clips], term)
        for i, pc in zip(clips, pad):
            ref = cs.restated_logprobs(("gpu-i", i), video[sel[i]], ids[sel[i], :pl].tolist(), [c.tolist() for c in cands[i]], term, sd, cfg)
            for j, lp in enumerate(pc):
                assert int(res[i]["count"][j]) == len(lp)
                e_padded = max(e_padded, (lp.double() - ref[j]).abs().max().item())
                e_packed = max(e_packed, (res[i]["token_logprob"][j, :len(lp)].double() - ref[j]).abs().max().item())
    print(f"    (i) padded forward_continuation: e_packed {e_packed:.3e} e_padded {e_padded:.3e}")
    assert e_packed <= 1.5 * e_padded + 1e-6, (e_packed, e_padded)
    # (ii)
    N = 4
    text2 = cs.text_of(ids, mask, [0, 1], dev)
    out, scores = model.generate(vid, text2, termination_id=term, do_sample=True, num_samples=N, return_scores=True, seed=11)
    e_pk = e_smp = 0.0
    for ended in (True, False):
        cl, where = [], []
        for i in range(2):
            pl = int(mask[i].sum()) - 1
            cl.append([])
            for s in range(N):
                gen = out[i][s, pl:].tolist()
                if (term in gen) != ended:
                    continue
                cl[-1].append(gen[:gen.index(term)] if ended else gen)
                where.append((i, s, pl))
        if not where:
            continue
        rs = model.score_captions(vid, text2, cl, termination_id=term, score_termination=ended)
        at = [0, 0]
        for i, s, pl in where:
            j = at[i]
            at[i] += 1
            n = int(scores[i]["count"][s])
            assert int(rs[i]["count"][j]) == n, (i, s, ended)
            toks = out[i][s, pl:pl + n].tolist()
            ref = cs.restated_logprobs(("gpu-ii", i, s), video[i], ids[i, :pl].tolist(), [toks[:-1]], toks[-1], sd, cfg)[0]
            e_smp = max(e_smp, (scores[i]["token_logprob"][s, pl:pl + n].double() - ref).abs().max().item())
            e_pk = max(e_pk, (rs[i]["token_logprob"][j, :n].double() - ref).abs().max().item())
    print(f"    (ii) the sampler's own scores: e_packed {e_pk:.3e} e_sampled {e_smp:.3e}")
    assert e_pk <= 1.5 * e_smp + 1e-6, (e_pk, e_smp)
    # (iii)
    worst = golden_anchor(model, cfg, g, sd, video, ids, mask, dev, PLAIN["caption_tiny"]["score"])
    print(f"    (iii) golden anchor: worst relative deviation {worst:.3e} <= {PLAIN['caption_tiny']['score']:.1e}")


# ------------------------------------------------------------------------------ the entry point
def run_entrypoint_with_and_without_the_flag(tmp_path, more=()):
    """--synthetic_steps --evaluate_only with --eval_score_gold: the result entries carry gold_logprob / gold_tokens (one per gold caption)
    and the log a finite perplexity; the flag defaults off, and the run without it writes the result file of the flagged run minus the
    new lists, byte for byte (same seed: the flag changes nothing else)."""
    import test_entrypoint_gpu as t
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    os.makedirs(str(tmp_path), exist_ok=True)
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    files = {}
    for name, flags in (("plain", list(more)), ("gold", list(more) + ["--eval_score_gold"])):
        out = str(tmp_path / name)
        base = ["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only"]
        args, config = entry.get_args(base + flags)
        assert args.eval_score_gold == (name == "gold")
        stats = entry.main(args, config)
        files[name] = open(os.path.join(out, "result", "val_caption_result.json")).read()
        if name == "gold":
            assert math.isfinite(stats["val_gold_ppl"]) and stats["val_gold_ppl"] > 1.0 and stats["val_gold_nll"] > 0 and stats["val_gold_scored_tokens"] > 0
            log = json.loads(open(os.path.join(out, "log.txt")).read().strip().splitlines()[-1])
            assert math.isfinite(log["val_gold_ppl"]) and log["val_gold_ppl"] == pytest.approx(math.exp(log["val_gold_nll"]))
        else:
            assert not any("gold" in k for k in stats)
    plain, gold = json.loads(files["plain"]), json.loads(files["gold"])
    keys = {"video_id", "pred_caption", "gold_caption"} | ({"sampled_captions"} if "--eval_sample" in more else set())
    assert len(gold) == len(plain) == 5 and all(set(r) == keys for r in plain)
    for r in gold:
        assert set(r) == keys | {"gold_logprob", "gold_tokens"}
        assert len(r["gold_logprob"]) == len(r["gold_tokens"]) == len(r["gold_caption"]) == 2
        assert all(math.isfinite(x) and x < 0 for x in r["gold_logprob"])
        assert r["gold_tokens"] == [len(c) + 1 for c in r["gold_caption"]]          # one token per character + the terminator
    stripped = [{k: v for k, v in r.items() if k not in ("gold_logprob", "gold_tokens")} for r in gold]
    assert json.dumps(stripped) == files["plain"]
    return gold


@gpu
def test_caption_entrypoint_scores_the_gold_captions(tmp_path, dev):
    run_entrypoint_with_and_without_the_flag(tmp_path / "a")
    # beside the lockstep search on the shared-prefix KV cache and sampled captions: the flag combines with the other evaluation flags
    run_entrypoint_with_and_without_the_flag(tmp_path / "b", more=["--eval_batched_beam", "--eval_shared_kv", "--eval_sample", "2"])
