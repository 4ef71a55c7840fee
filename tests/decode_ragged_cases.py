"""Cases of the ragged shared-prefix decode tests (tests/test_decode_ragged_gpu.py): the attention operands with a prefix length per
group, laid out as the real caches are, and the state case on the tiny decoder."""
import torch

import standin_decode_ragged as sr
import standin_decode_shared as sd

BF = torch.bfloat16

# (head_dim, heads, group_size, lengths per group, own_len, sequences the last group is short of): the 32-key tile and 128-key chunk
# edges (1, 31 / 32 / 33, 127 .. 130, 259 / 264 / 270), groups whose prefix tile counts differ mod 4 next to each other (the wave that
# runs a row's own tiles is (prefix tiles + row) % 4), one and two own tiles per row, two row tiles, a short last group
SWEEP = [
    (64, 2, 5, [1, 32, 33, 129], 1, 0),
    (64, 1, 5, [264, 259, 270], 12, 0),
    (80, 1, 8, [65, 31, 128], 33, 0),
    (64, 1, 33, [33, 1], 2, 0),
    (80, 2, 3, [127, 128, 129, 130, 96], 32, 1),
]


def case_id(c):
    return f"hd{c[0]}-h{c[1]}-g{c[2]}-L{'_'.join(map(str, c[3]))}-own{c[4]}-short{c[5]}"


def make_case(hd, heads, group_size, lengths, own_len, short_last=0, seed=0, device="cpu", prefix_pad=0.0, suffix_pad=0.0):
    """standin_decode_shared.make_case with the pitch max(lengths) between two groups' prefixes; group g's prefix rows at and beyond
    lengths[g] hold `prefix_pad`, suffix rows at and beyond own_len `suffix_pad`.  -> its dict plus lengths and group_prefix_len
    (int32, on the device)"""
    pitch = max(lengths)
    c = sd.make_case(hd, heads, len(lengths), group_size, pitch, own_len, short_last, suffix_max=own_len + 3, seed=seed, device=device,
                     pad=suffix_pad)
    rows = c["prefix"].view(len(lengths), pitch, 3 * heads * hd)
    for g, n in enumerate(lengths):
        rows[g, n:] = prefix_pad
    return dict(c, lengths=list(lengths), group_prefix_len=torch.tensor(lengths, dtype=torch.int32, device=device))


def reference(c):
    """the fp32 softmax over each group's first lengths[g] prefix keys followed by the sequence's own keys"""
    return sr.attn_decode_shared_ragged_ref(*[c[n] for n in ("q", "k", "v", "pk", "pv", "lay", "prefix_lay", "n_seq", "group_size", "heads",
                                                             "lengths", "own_len", "hd", "scale")])


def group_alone(c, g):
    """the uniform entry's case for group g alone with prefix_len = its own length (the operands are views of c's)"""
    gs, S, P, H = c["group_size"], c["S"], c["prefix_len"], c["heads"] * c["hd"]
    n = min(gs, c["n_seq"] - g * gs)
    off = g * gs * S * 3 * H
    return dict(c, n_seq=n, o=torch.zeros(n, H, dtype=BF, device=c["o"].device), q=c["q"][off:], k=c["k"][off:], v=c["v"][off:],
                pk=c["pk"][g * P * 3 * H:], pv=c["pv"][g * P * 3 * H:], prefix_len=c["lengths"][g])


# ------------------------------------------------------------------------------------------------ the state on the tiny decoder
PROMPTS, FAN, Q, STEPS = [2, 5, 9], 3, 8, 6
PERMS = ([0, 0, 1], [2, 1, 1], [1, 2, 0])                     # in-group re-orders, the same in every clip


def state_inputs(cfg, dev):
    g = torch.Generator().manual_seed(33)
    G = len(PROMPTS)
    qe = (torch.randn(G, Q, cfg.hidden, generator=g) * 0.5).to(dev).to(BF)
    prompt = torch.randint(0, cfg.vocab, (G, max(PROMPTS)), generator=g)
    for c, n in enumerate(PROMPTS):
        prompt[c, n:] = 7                                     # right-padded behind the real tokens
    toks = [torch.randint(0, cfg.vocab, (G * FAN, 1), generator=g).to(dev) for _ in range(2 + len(PERMS))]
    return qe, prompt.to(dev), toks


def run_ragged_state(gpt, dev, qe, prompt, toks, weights="bf16", poison=False):
    """three clips with prompts of 2 / 5 / 9 tokens, fan 3: the prefill, two steps, then three steps after in-group re-orders ->
    the logits of the six calls, and the state.  poison: after the prefill the prefix cache's rows behind every clip's prompt --
    the KV of the pad rows -- are overwritten with NaN."""
    from youku_mplug_amd.generation import SharedPrefixDecodeState
    G = len(PROMPTS)
    st = SharedPrefixDecodeState(gpt, G * FAN, Q + max(PROMPTS) + STEPS, weights)
    out = [st.prefill_fan_out(prompt, qe, FAN, prompt_len=torch.tensor(PROMPTS))]
    if poison:
        rows = st.prefix.cache.view(st.nl, G, st.P, -1)
        for c, n in enumerate(PROMPTS):
            rows[:, c, Q + n:] = float("nan")
    for i, tok in enumerate(toks):
        if i >= 2:
            perm = torch.tensor([c * FAN + j for c in range(G) for j in PERMS[i - 2]], device=dev)
            st.reorder(perm, shared_prefix=st.P)
        out.append(st.step(tok))
    return out, st


def run_uniform_states(gpt, dev, qe, prompt, toks):
    """the same six calls clip by clip on uniform SharedPrefixDecodeStates (one per clip, its own prompt length) -> the logits
    assembled in the ragged state's row order"""
    from youku_mplug_amd.generation import SharedPrefixDecodeState
    per_clip = []
    for c, n in enumerate(PROMPTS):
        st = SharedPrefixDecodeState(gpt, FAN, Q + n + STEPS)
        out = [st.prefill_fan_out(prompt[c:c + 1, :n].contiguous(), qe[c:c + 1].contiguous(), FAN)]
        for i, tok in enumerate(toks):
            if i >= 2:
                st.reorder(torch.tensor(PERMS[i - 2], device=dev), shared_prefix=Q + n)
            out.append(st.step(tok[c * FAN:(c + 1) * FAN].contiguous()))
        per_clip.append(out)
    return [torch.cat([per_clip[c][i] for c in range(len(PROMPTS))], dim=0) for i in range(len(toks) + 1)]
