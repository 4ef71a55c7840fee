"""Shared by tests/test_caption_score_cpu.py and tests/test_caption_score_gpu.py: the length lists and groupings of the packed
attention sweep, a Python restatement of mpv_attn_prefix_packed_layout, the tiny caption model of tests/golden/caption_tiny.pt, the fp32
restatement's teacher-forced log-probabilities (oracle.restate: the yardstick every path is compared with) and the padded
forward_continuation pass on the same candidates."""
import os
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# (continuation lengths, continuations per group) of the kernel sweep: every length list under one group and under all-ones, and mixes
# that put a group of more than 128 rows next to one of fewer
LENGTHS = [[1], [128], [129], [1, 127, 1], [33, 31, 32, 32, 5], [7] * 19, [300]]
LAYOUTS = [(l, [len(l)]) for l in LENGTHS] + [(l, [1] * len(l)) for l in LENGTHS if len(l) > 1] + [
    ([1, 127, 1], [2, 1]),                      # 128 rows | 1 row
    ([33, 31, 32, 32, 5], [3, 2]),              # 96 | 37
    ([33, 31, 32, 32, 5, 300], [3, 1, 2]),      # 96 | 32 | 305: a group of more than 128 rows behind two of fewer
    ([7] * 19 + [3], [19, 1]),                  # 133 | 3
    ([300, 2, 129], [1, 1, 1]),
]


def layout_id(l):
    return "L" + "-".join(str(x) for x in (l[0] if len(set(l[0])) > 1 or len(l[0]) < 4 else [f"{l[0][0]}x{len(l[0])}"])) + "_G" + "-".join(
        str(x) for x in (l[1] if len(set(l[1])) > 1 or len(l[1]) < 4 else [f"{l[1][0]}x{len(l[1])}"]))


def layout_restated(cont_len, conts_per_group):
    """(seg_start, group_row, rows, max_group_rows) as include/mpv.h defines them"""
    seg, grp, c = [], [0], 0
    for n in conts_per_group:
        for _ in range(n):
            seg += [len(seg)] * cont_len[c]
            c += 1
        grp.append(len(seg))
    return seg, grp, len(seg), max(b - a for a, b in zip(grp, grp[1:]))


def tiny_caption_model(dev):
    """the model, inputs and golden record of tests/test_model_gpu.py:test_caption_generate_vs_reference_golden"""
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict
    from youku_mplug_amd.downstream import synthetic_gencls_model
    g = torch.load(os.path.join(GOLD, "caption_tiny.pt"))
    m = g["meta"]
    model = synthetic_gencls_model(CONFIG_TINY, "caption", device=dev)
    sd = make_state_dict(CONFIG_TINY, m["weight_seed"])
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    model.text_decoder.config.extra.update(tokens_to_generate=m["tokens_to_generate"], eod_id=m["eod_id"])
    video, ids, mask = make_inputs(CONFIG_TINY, m["batch"], m["text_len"], seed=m["input_seed"], ragged=False)
    mask[1, 4:] = 0
    return model.eval(), CONFIG_TINY, g, sd, video, ids, mask


def text_of(ids, mask, sel, dev):
    return types.SimpleNamespace(input_ids=ids[sel].to(dev), attention_mask=mask[sel].to(dev))


def ragged_candidates(cfg, counts, seed, lo=1, hi=9, avoid=None):
    """counts[i] candidates for clip i with lengths in [lo, hi], tokens drawn from the vocabulary without `avoid` (the terminator)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in counts:
        cl = []
        for _ in range(n):
            ln = int(torch.randint(lo, hi + 1, (1,), generator=g))
            t = torch.randint(0, cfg.vocab, (ln,), generator=g)
            if avoid is not None:
                t[t == avoid] = (avoid + 1) % cfg.vocab
            cl.append(t)
        out.append(cl)
    return out


_restated = {}


def restated_logprobs(key, video, prompt, cands, term, sd, cfg, weights="bf16"):
    """fp32 restatement (oracle.restate.pretrain_forward), teacher-forced: for every candidate c of ONE clip the log-probabilities of
    [c_0 .. c_{n-1}, term] after `prompt` (a list of token ids).  One decoder batch per clip: the candidates are padded on the right with
    `term`, which a causal decoder does not see from the scored positions.  weights="bf16": the state dict rounded to bf16 (what the
    model under test holds); "fp32": as it is (the golden's fp32 run).  Cached by `key`: computed once, shared, never modified."""
    from oracle import restate
    if key in _restated:
        return _restated[key]
    sdr = {k: v.bfloat16().float() for k, v in sd.items()} if weights == "bf16" else {k: v.float() for k, v in sd.items()}
    vid = video.bfloat16().float() if weights == "bf16" else video.float()
    Q, pl = cfg.num_queries, len(prompt)
    W = pl + max(len(c) for c in cands) + 1
    ids = torch.tensor([list(prompt) + list(c) + [term] * (W - pl - len(c)) for c in cands], dtype=torch.long)
    with torch.no_grad():
        out = restate.pretrain_forward(vid[None].expand(len(cands), *vid.shape).contiguous(), ids, torch.ones_like(ids), sdr, cfg)
    lp = torch.log_softmax(out["logits"].double(), dim=-1)                  # [C, Q + W, V]
    res = []
    for j, c in enumerate(cands):
        tgt = torch.tensor(list(c) + [term], dtype=torch.long)
        rows = Q + pl - 1 + torch.arange(len(tgt))
        res.append(lp[j, rows, tgt].clone())
    _restated[key] = res
    return res


def padded_logprobs(model, qf, ids_dev, pl, cands, term):
    """The existing padded path on the same candidates: forward_prefix over Q + prompt[:-1] of every clip, then forward_continuation with
    every candidate padded to the chunk's longest (the clips share the prompt length pl and the number of candidates).  -> per clip,
    per candidate a CPU fp32 tensor of the log-probabilities of [c_0 .. c_{n-1}, term]."""
    dec = model.text_decoder
    n, t = len(cands), len(cands[0])
    assert all(len(cl) == t for cl in cands)
    Lc = max(len(c) for cl in cands for c in cl) + 1
    dev = qf.device
    rows_in, loss_rows, labels = [], [], []
    for i, cl in enumerate(cands):
        last = int(ids_dev[i, pl - 1])
        for j, c in enumerate(cl):
            c = [int(x) for x in c]
            rows_in.append([last] + c + [term] * (Lc - 1 - len(c)))
            loss_rows += [(i * t + j) * Lc + p for p in range(len(c) + 1)]
            labels += c + [term]
    prefix = dec.forward_prefix(qf.reshape(-1, qf.shape[-1]).contiguous(), ids_dev[:, :pl - 1].contiguous())
    out = dec.forward_continuation(prefix, torch.tensor(rows_in, dtype=torch.long, device=dev), t,
                                   loss_rows=torch.tensor(loss_rows, dtype=torch.long, device=dev),
                                   labels=torch.tensor(labels, dtype=torch.long, device=dev))
    lp, at, res = (-out["losses"]).float().cpu(), 0, []
    for cl in cands:
        res.append([])
        for c in cl:
            res[-1].append(lp[at:at + len(c) + 1].clone())
            at += len(c) + 1
    return res
