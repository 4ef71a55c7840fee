"""The fused sampler on the GPU: mpv_sample_advance (csrc/sampling.hip) against its fp64 restatement tests/standin_sampling.py on every
committed case of tests/sampling_cases.py (token and kept-set size equal on every row, kept mass within 1e-5, canaries behind every
output), the two ends of the uniform, greedy against mpv_logprob_topk, the counter-based uniform, determinism and independence of the
launch, the distribution of 8192 draws, the bookkeeping of six steps in each termination mode, every refusal, and on the tiny model
sample_batched / DistributedGPT3_Caption.generate(do_sample=True)."""
import ctypes as C
import math
import os
import types

import pytest
import torch

import sampling_cases as sc
import standin_sampling as ss

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY = 64


class _Guarded:
    """a device array with CANARY elements behind it that must stay what they are"""

    def __init__(self, n, dtype, dev, fill):
        self.mark = {torch.int32: -77, torch.int64: -7777, torch.float32: -7.5}[dtype]
        self.buf = torch.full((n + CANARY,), self.mark, dtype=dtype, device=dev)
        self.t = self.buf[:n]
        self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[self.t.numel():] == self.mark).all())


def _state(dev, rows, row_len=sc.ROW_LEN, prompt_len=None, streams=None, fill=3):
    """a SampleState whose arrays all have canaries behind them -> (state, guards)"""
    from youku_mplug_amd.generation import SampleState
    st = SampleState(torch.full((rows, row_len), fill, dtype=torch.int64, device=dev),
                     torch.zeros(rows, dtype=torch.int64, device=dev) if prompt_len is None else prompt_len.to(dev), streams=streams)
    guards = {}
    for name, n, dt in (("tokens", rows * row_len, torch.int64), ("done", rows, torch.int32), ("next_tok", rows, torch.int64), ("n_done", 1, torch.int32)):
        g = _Guarded(n, dt, dev, 0)
        g.t.copy_(getattr(st, name).reshape(-1))
        setattr(st, name, g.t.view(getattr(st, name).shape))
        guards[name] = g
    return st, guards


def _outs(dev, rows):
    return {"out_token": _Guarded(rows, torch.int64, dev, -1), "out_kept": _Guarded(rows, torch.int32, dev, -1), "out_mass": _Guarded(rows, torch.float32, dev, -1.0)}


def _run(dev, logits, vocab, T, filt, *, seed=0, pos=sc.POS, u=None, streams=None):
    from youku_mplug_amd import ops
    rows = logits.shape[0]
    st, guards = _state(dev, rows, streams=streams)
    outs = _outs(dev, rows)
    top_k, top_p = sc.filter_args(filt)
    ops.sample_advance(logits, st, pos=pos, temperature=T, top_k=top_k, top_p=top_p, seed=seed, vocab=vocab, termination_id=-1,
                       u_override=None if u is None else u.to(dev), **{k: g.t for k, g in outs.items()})
    torch.cuda.synchronize()
    assert all(g.intact() for g in list(guards.values()) + list(outs.values())), "a canary behind an output array was overwritten"
    return {k: g.t.cpu() for k, g in outs.items()}, st


_REF = {}


def _reference(i):
    """the stand-in's answer for committed case i, computed once and shared"""
    if i not in _REF:
        V, rows, ld, seed, T, filt, skip = sc.CASES[i]
        logits, _ = sc.case_rows(sc.CASES[i])
        top_k, top_p = sc.filter_args(filt)
        res = [ss.sample_row(logits[r, :V], T, top_k, top_p, ss.uniform(seed, sc.POS, r)) for r in range(rows)]
        _REF[i] = (logits, torch.tensor([r["token"] for r in res]), torch.tensor([r["kept"] for r in res], dtype=torch.int32),
                   torch.tensor([r["mass"] for r in res], dtype=torch.float64))
    return _REF[i]


@pytest.mark.parametrize("V", [8, 64, 8000, 51200, 65536])
def test_kernel_equals_the_standin_on_every_listed_case(dev, V):
    """out_token and out_kept equal on EVERY row, out_mass within 1e-5; the token lands in column POS of the table and in next_tok; the
    columns behind `vocab` (poison) are never drawn; canaries intact (checked in _run)."""
    n = 0
    for i, case in enumerate(sc.CASES):
        if case[0] != V:
            continue
        _, rows, ld, seed, T, filt, _ = case
        logits, tok, kept, mass = _reference(i)
        got, st = _run(dev, logits.to(dev), V, T, filt, seed=seed)
        worst = (got["out_mass"].double() - mass).abs().max().item()
        print(f"    V={V} rows={rows} ld={ld} T={T} {filt}: kept mass error {worst:.2e}")
        assert torch.equal(got["out_token"], tok), (case[:6], (got["out_token"] != tok).nonzero().view(-1).tolist()[:8])
        assert torch.equal(got["out_kept"], kept), (case[:6], (got["out_kept"] != kept).nonzero().view(-1).tolist()[:8])
        assert worst <= 1e-5, (case[:6], worst)
        assert torch.equal(st.tokens[:, sc.POS].cpu(), tok) and torch.equal(st.next_tok.cpu(), tok)
        assert (st.tokens.cpu()[:, [c for c in range(sc.ROW_LEN) if c != sc.POS]] == 3).all() and int(st.n_done.item()) == 0
        n += 1
    assert n >= 7


# rows for the two ends of the uniform: (V, row seed, variant, T, filter).  u = 0 picks the first kept index exactly.  u = 1 - 2^-24 picks
# the last kept index when that index carries more than 2 * DELTA of the kept mass (asserted on the reference below: these rows do, the
# kept sets of top-k 2 / top-p on them being hot entries or a tie group); with a last index of mass ~1e-9 fp32 could not tell.
END_ROWS = [(8, 11, "normal", 1.0, ("top_k", 2)), (8, 12, "all_equal", 1.0, ("plain",)), (64, 13, "cutoff_ties", 0.7, ("top_p", 0.5)),
            (64, 14, "normal", 1.0, ("top_p", 0.9)), (8000, 15, "normal", 1.5, ("top_k", 2)), (8000, 16, "cutoff_ties", 1.0, ("top_p", 0.9)),
            (51200, 17, "normal", 1.0, ("top_p", 0.9)), (51200, 18, "half_neg_inf", 1.0, ("top_k", 2)), (51200, 19, "cutoff_ties", 1.0, ("top_k", 2)),
            (65536, 20, "normal", 0.7, ("top_p", 0.5)), (65536, 21, "one_hot", 1.0, ("top_p", 0.9)), (65536, 22, "cutoff_ties", 1.3, ("top_p", 0.5))]


def test_the_two_ends_of_the_uniform_hit_the_first_and_the_last_kept_index(dev):
    for V, row_seed, variant, T, filt in END_ROWS:
        row = sc.make_row(V, row_seed, variant)
        top_k, top_p = sc.filter_args(filt)
        for u in (0.0, 1.0 - 2.0 ** -24):
            ref = ss.sample_row(row, T, top_k, top_p, u)
            idx = ref["kept_mask"].nonzero().view(-1)
            pk = ref["p"][ref["kept_mask"]]
            want = int(idx[0] if u == 0.0 else idx[-1])
            assert ref["token"] == want and float(pk[-1] / pk.sum()) > 2 * sc.DELTA and float(pk[0]) > 0.0
            got, _ = _run(dev, row[None].to(dev), V, T, filt, u=torch.tensor([u], dtype=torch.float32))
            assert int(got["out_token"][0]) == want and int(got["out_kept"][0]) == ref["kept"], (V, variant, filt, u)


def test_greedy_equals_logprob_topk_on_rows_full_of_ties(dev):
    from youku_mplug_amd import ops
    g = torch.Generator().manual_seed(5)
    for V, rows in ((64, 5), (8000, 5), (51200, 16)):
        logits = (torch.randint(-8, 9, (rows, V), generator=g).float() / 4).to(torch.bfloat16).to(dev)      # 33 values: the maximum is tied ~V / 33 times
        got, _ = _run(dev, logits, V, 1.0, ("greedy",))
        want = ops.logprob_topk(logits, 1)[1].view(-1).cpu()
        assert torch.equal(got["out_token"], want) and (got["out_kept"] == 1).all()
        assert torch.equal(want, torch.argmax((logits.float().cpu() == logits.float().cpu().max(dim=1, keepdim=True).values).int(), dim=1))


def test_uniform_determinism_and_independence_of_the_launch(dev):
    """the RNG path equals the u_override path fed with standin_sampling.uniform, bit for bit; two runs are bit-identical; a row draws
    the same alone (with its stream) as inside the 160-row launch; another seed / pos / stream draws something else somewhere"""
    i = next(i for i, c in enumerate(sc.CASES) if c[:2] == (51200, 160) and c[5][0] == "top_p")
    V, rows, ld, seed, T, filt, _ = sc.CASES[i]
    logits = _reference(i)[0].to(dev)
    a, _ = _run(dev, logits, V, T, filt, seed=seed)
    b, _ = _run(dev, logits, V, T, filt, seed=seed)
    u = torch.tensor([ss.uniform(seed, sc.POS, r) for r in range(rows)], dtype=torch.float32)
    assert all(float(x) == ss.uniform(seed, sc.POS, r) for r, x in enumerate(u))                   # 24 bits: exact in fp32
    c, _ = _run(dev, logits, V, T, filt, seed=seed + 99, u=u)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    for r in (0, 37, 159):
        alone, _ = _run(dev, logits[r:r + 1], V, T, filt, seed=seed, streams=torch.tensor([r]))
        for k in a:
            assert torch.equal(alone[k], a[k][r:r + 1]), (r, k)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(1))
    moved, _ = _run(dev, logits[perm.to(dev)].contiguous(), V, T, filt, seed=seed, streams=perm)       # rows shuffled, streams with them
    for k in a:
        assert torch.equal(moved[k], a[k][perm]), k
    for kw in (dict(seed=seed + 1), dict(seed=seed, pos=sc.POS + 1), dict(seed=seed, streams=torch.arange(rows) + 1000)):
        other, _ = _run(dev, logits, V, T, filt, **kw)
        assert not torch.equal(other["out_token"], a["out_token"]), kw
        assert torch.equal(other["out_kept"], a["out_kept"]) and torch.equal(other["out_mass"], a["out_mass"])      # the filter does not see u


def test_distribution_of_8192_draws(dev):
    """one launch of 8192 rows with the same V = 64 logits, plain sampling, streams 0 .. 8191: every token's count within
    5 * sqrt(n p (1 - p)) + 1 of n p, p from fp64 -- the binomial's bound, deterministic for this seed"""
    n, V, T = 8192, 64, 1.0
    row = sc.make_row(V, 4242, "normal")
    p = torch.softmax(row.double() / T, dim=-1)
    got, _ = _run(dev, row[None].repeat(n, 1).to(dev), V, T, ("plain",), seed=20240)
    counts = torch.bincount(got["out_token"], minlength=V).double()
    bound = 5 * torch.sqrt(n * p * (1 - p)) + 1
    worst = ((counts - n * p).abs() / bound).max().item()
    print(f"    worst |count - n p| / bound = {worst:.3f}; tokens drawn: {int((counts > 0).sum())}")
    assert ((counts - n * p).abs() <= bound).all(), (counts - n * p).abs().max().item()
    assert int((counts > 0).sum()) >= 20


def _scripted_logits(script_col, V=640):
    """[rows, V] bf16: the tail of a normal row with +12 at the scripted token -- a nucleus of one"""
    out = torch.stack([sc.make_row(V, 50 + r, "normal").float() for r in range(len(script_col))])
    for r, t in enumerate(script_col):
        out[r, t] = 12.0
    return out.to(torch.bfloat16)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bookkeeping_of_six_steps_equals_the_standin(dev, mode):
    """3 rows, ragged prompt lengths (one row is still teacher-forced for two steps), row 2 marked done beforehand, top-p 0.9 at T = 1.1:
    tokens, done, next_tok and n_done equal the stand-in bit for bit after every step"""
    from youku_mplug_amd import ops
    from youku_mplug_amd.generation import SampleState
    script = [[9, 198, 198, 5, 628, 9], [5, 5, 198, 198, 9, 5], [5, 9, 5, 198, 5, 628]]
    prompt_len = torch.tensor([2, 4, 1])
    table = torch.randint(0, 600, (3, 10), generator=torch.Generator().manual_seed(mode))
    table[1, 2], table[1, 3] = 198, 7                                          # prompt tokens of the teacher-forced row
    ref = SampleState(table.clone(), prompt_len)
    mine, guards = _state(dev, 3, row_len=10, prompt_len=prompt_len)
    mine.tokens.copy_(table.to(dev))
    ref.done[2], mine.done[2] = 1, 1
    kw = dict(temperature=1.1, top_k=0, top_p=0.9, seed=77, vocab_size=640, termination_mode=mode, termination_id=9)
    seen_done = []
    for step in range(6):
        pos = 2 + step
        logits = _scripted_logits([s[step] for s in script])
        ss.sample_advance(logits, ref, pos=pos, **kw)
        ops.sample_advance(logits.to(dev), mine, pos=pos, **kw)
        torch.cuda.synchronize()
        for name in ("tokens", "done", "next_tok", "n_done", "prompt_len", "stream"):
            assert torch.equal(getattr(mine, name).cpu(), getattr(ref, name)), (mode, step, name)
        assert all(g.intact() for g in guards.values())
        seen_done.append(int(ref.n_done))
    assert ref.tokens[1, 2] == 198 and ref.tokens[1, 3] == 7                  # teacher forcing kept the prompt
    assert ref.tokens[0, 2:8].tolist() == script[0] and ref.tokens[1, 4:8].tolist() == script[1][2:] and ref.tokens[2, 2:8].tolist() == script[2]
    # by hand: id 9 -- row 0 at step 0, row 1 at step 4; eol -- row 0 at step 1, row 1 at step 2 (its first own token); double eol --
    # row 0 at step 2, row 1 at step 3 (198 at step 2 follows the prompt's 7); row 2 was done all along
    assert seen_done == {0: [2, 2, 2, 2, 3, 3], 1: [1, 2, 3, 3, 3, 3], 2: [1, 1, 2, 3, 3, 3]}[mode], seen_done


def test_refusals_leave_everything_untouched(dev):
    """one call per rule of the header's list: a negative code before any launch, state and outputs unchanged"""
    from youku_mplug_amd import _lib, ops
    logits = sc.make_row(64, 1, "normal")[None].repeat(2, 1).to(dev)
    st, guards = _state(dev, 2)
    outs = _outs(dev, 2)
    before = {k: g.buf.clone() for k, g in {**guards, **outs}.items()}
    good = dict(pos=1, temperature=1.0, top_k=0, top_p=0.0, **{k: g.t for k, g in outs.items()})
    nan, inf = float("nan"), float("inf")
    rules = [("vocab % 8", dict(vocab=60)), ("vocab < 8", dict(vocab=0)), ("vocab > 65536", dict(vocab=65544, ld=65544)), ("ld < vocab", dict(ld=56)),
             ("ld % 8", dict(ld=68)), ("T = 0", dict(temperature=0.0)), ("T < 0", dict(temperature=-1.0)), ("T = inf", dict(temperature=inf)),
             ("T = nan", dict(temperature=nan)), ("top_k > 1 with top_p", dict(top_k=5, top_p=0.9)), ("greedy with top_p", dict(top_k=1, top_p=0.9)),
             ("top_k > vocab", dict(top_k=65)), ("top_k < 0", dict(top_k=-1)), ("top_p > 1", dict(top_p=1.5)), ("top_p < 0", dict(top_p=-0.1)),
             ("pos = row_len", dict(pos=sc.ROW_LEN)), ("pos < 0", dict(pos=-1)), ("termination_mode", dict(termination_mode=3))]
    for what, bad in rules:
        d = ops.sample_advance_desc(logits, st, **{**good, **bad})
        rc = _lib.lib().mpv_sample_advance(C.byref(d), ops._stream())
        assert rc < 0 and b"mpv_sample_advance" in _lib.lib().mpv_last_error(), (what, rc)
    for field in ("logits", "tokens", "prompt_len", "done", "next_tok", "n_done"):
        d = ops.sample_advance_desc(logits, st, **good)
        setattr(d, field, None)
        assert _lib.lib().mpv_sample_advance(C.byref(d), ops._stream()) < 0, field
    assert _lib.lib().mpv_sample_advance(None, ops._stream()) < 0
    misaligned = torch.zeros(2 * 64 + 8, dtype=torch.bfloat16, device=dev)[1:1 + 128].view(2, 64)
    d = ops.sample_advance_desc(misaligned, st, **good)
    assert _lib.lib().mpv_sample_advance(C.byref(d), ops._stream()) < 0
    with pytest.raises(_lib.MpvError, match="top-k and top-p"):
        ops.sample_advance(logits, st, **{**good, "top_k": 5, "top_p": 0.9})
    with pytest.raises(_lib.MpvError):
        ops.sample_advance(logits.float(), st, **good)
    torch.cuda.synchronize()
    for k, g in {**guards, **outs}.items():
        assert torch.equal(g.buf, before[k]), k
    ops.sample_advance(logits, st, **good)                                     # and the good call goes through
    torch.cuda.synchronize()
    assert (outs["out_kept"].t == 64).all() and (outs["out_token"].t >= 0).all()
    toks = ops.sample_tokens(logits, top_k=1)
    assert torch.equal(toks.cpu(), torch.argmax(logits.float().cpu(), dim=1))


# ------------------------------------------------------------------------------ on the tiny model
def _caption_model(dev):
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict
    from youku_mplug_amd.downstream import synthetic_gencls_model
    m = torch.load(os.path.join(GOLD, "caption_tiny.pt"))["meta"]
    model = synthetic_gencls_model(CONFIG_TINY, "caption", device=dev)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in make_state_dict(CONFIG_TINY, m["weight_seed"]).items()}, strict=True)
    model.text_decoder.config.extra.update(tokens_to_generate=m["tokens_to_generate"], eod_id=m["eod_id"])
    video, ids, mask = make_inputs(CONFIG_TINY, m["batch"], m["text_len"], seed=m["input_seed"], ragged=False)
    return m, model, video.to(dev).to(torch.bfloat16), ids, mask


def test_greedy_sample_batched_equals_sample_on_the_tiny_model(dev):
    """sample_batched(top_k = 1) against today's sample(top_k = 1): ragged prompt lengths and a visual prefix, token for token"""
    from oracle.weights import CONFIG_TINY
    m, model, video, ids, mask = _caption_model(dev)
    td = model.text_decoder
    td.config.extra.update(top_k=1, top_p=0.0)
    g = torch.Generator().manual_seed(8)
    B, Q = 3, 6
    qe = (torch.randn(B, Q, CONFIG_TINY.hidden, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    tokens = torch.randint(0, CONFIG_TINY.vocab, (B, 5), generator=g).to(dev)
    lengths = torch.tensor([5, 2, 3], device=dev)
    model.eval()
    with torch.no_grad():
        want = td.sample(tokens.clone(), query_embeds=qe, prompt_length=lengths.clone(), termination_id=m["eod_id"])
        got = td.sample_batched(tokens.clone(), query_embeds=qe, prompt_length=lengths.clone(), termination_id=m["eod_id"])
        via = td.generate(tokens.clone(), query_embeds=qe, prompt_length=lengths.clone(), termination_id=m["eod_id"], sampler="device")
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert torch.equal(via, want)
    for b in range(B):
        assert torch.equal(got[b, :int(lengths[b])], tokens[b, :int(lengths[b])])


def test_caption_generate_do_sample_on_the_tiny_model(dev):
    """generate(do_sample=True, num_samples=3, seed=s): per clip [3, Lt] in input order, every row continuing its prompt; the same per-clip
    result with clips_per_search 1, 2 and 32; with the clips permuted, the same stream per clip gives the same samples; without do_sample
    the call is the unchanged per-clip beam search."""
    m, model, video, ids, mask = _caption_model(dev)
    sel = [0, 1, 0]
    text = types.SimpleNamespace(input_ids=ids[sel].to(dev), attention_mask=mask[sel].to(dev))
    kw = dict(termination_id=m["eod_id"], do_sample=True, num_samples=3, seed=31, temperature=1.0, top_p=0.9)
    Lt, n_prompt = ids.shape[1] + m["tokens_to_generate"], int(mask[0].sum()) - 1
    base = model.generate(video[sel], text, **kw)
    assert len(base) == 3 and all(r.shape == (3, Lt) and r.dtype == torch.int64 and not r.is_cuda for r in base)
    for i, r in enumerate(base):
        assert (r[:, :n_prompt] == ids[sel[i], :n_prompt]).all(), i
    assert len({tuple(row) for r in base for row in r.tolist()}) > 3           # samples differ
    for cps in (1, 2):
        res = model.generate(video[sel], text, clips_per_search=cps, **kw)
        assert all(torch.equal(a, b) for a, b in zip(res, base)), cps
    again = model.generate(video[sel], text, **kw)
    assert all(torch.equal(a, b) for a, b in zip(again, base))
    # permuted clips with their streams: the decoder's own entry point
    td = model.text_decoder
    model.eval()
    with torch.no_grad():
        qf = model._query_features(video[[0, 1]], {"vit": {}, "pool": {}}).view(2, model.num_learnable_token, model.text_width)
        pl = torch.full((2,), n_prompt, device=dev)
        skw = dict(temperature=1.0, num_samples=3, seed=31, top_p=0.9, termination_id=m["eod_id"], use_eod_token_for_early_termination=False)
        fwd = td.sample_batched(ids[[0, 1]].to(dev), query_embeds=qf.contiguous(), prompt_length=pl, streams=torch.arange(6), **skw)
        rev = td.sample_batched(ids[[1, 0]].to(dev), query_embeds=qf[[1, 0]].contiguous(), prompt_length=pl, streams=torch.tensor([3, 4, 5, 0, 1, 2]), **skw)
    assert torch.equal(fwd[:3], rev[3:]) and torch.equal(fwd[3:], rev[:3])
    # without do_sample: the per-clip beam search, untouched
    calls = []
    orig = td.sample_batched
    td.sample_batched = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        plain = model.generate(video[sel], text, termination_id=m["eod_id"])
    finally:
        td.sample_batched = orig
    assert not calls and len(plain) == 3
    with torch.no_grad():
        for i in range(3):
            out = td.generate(text.input_ids[i:i + 1], query_embeds=qf[sel[i]:sel[i] + 1], termination_id=m["eod_id"], do_sample=False, prompt_length=n_prompt)
            assert torch.equal(plain[i], out.sequences.cpu()), i
