"""mpv_logits_guide on the GPU: the kernel, bit for bit on the whole [rows, ld] matrices, against the fp32
stand-in tests/standin_guidance.py on every case of tests/guidance_cases.py -- poison in the columns behind the vocabulary, a canary
behind both buffers, uncond unchanged --; a row alone against the row in a batch; two launches; the refusals; then the lockstep loops on
the tiny caption model under guidance against the same loop whose guide_fn is the stand-in run on the host, and
DistributedGPT3_Caption.generate(guidance_scale=) against the decoder entry."""
import ctypes as C
import types

import pytest
import torch

import guidance_cases as gc
import standin_guidance as stg

pytestmark = pytest.mark.gpu
CANARY = 64
MARK = -3.25


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _guarded(t, dev):
    """t on the device with CANARY marked elements behind it -> (the view, the whole buffer)"""
    buf = torch.full((t.numel() + CANARY,), MARK, dtype=torch.bfloat16, device=dev)
    view = buf[:t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _run(dev, case, b):
    """the case through ops.logits_guide -> (cond, uncond) on the CPU, the canaries checked"""
    from youku_mplug_amd import ops
    kw = dict(scale=case["scale"], alpha=case["alpha"], ban_value=case["ban"], vocab=case["V"])
    if b["whole"] is not None:                                               # cond and uncond: the halves of one allocation
        whole, buf = _guarded(b["whole"], dev)
        rows = b["cond"].shape[0]
        cond, uncond, bufs = whole[:rows], whole[rows:], [(buf, whole.numel())]
    else:
        (cond, cbuf), (uncond, ubuf) = _guarded(b["cond"], dev), _guarded(b["uncond"], dev)
        bufs = [(cbuf, cond.numel()), (ubuf, uncond.numel())]
    out = ops.logits_guide(cond, uncond, **kw)
    torch.cuda.synchronize()
    assert out is cond
    for buf, n in bufs:
        assert bool((buf[n:] == MARK).all()), "the canary behind a buffer was overwritten"
    return cond.cpu(), uncond.cpu()


@pytest.mark.parametrize("case", gc.KERNEL_CASES, ids=gc.case_id)
def test_kernel_equals_the_standin_bitwise(dev, case):
    b = gc.build(case)
    V = case["V"]
    uncond0 = b["uncond"].clone()
    got, got_u = _run(dev, case, b)
    want = stg.logits_guide(b["cond"].clone(), b["uncond"].clone(), scale=case["scale"], alpha=case["alpha"], ban_value=case["ban"], vocab=V)
    assert (got[:, V:] == gc.POISON).all() and (got_u[:, V:] == gc.POISON).all(), "a column behind the vocabulary was written"
    assert torch.equal(_bits(got_u), _bits(uncond0)), "uncond was written"
    diff = (_bits(got) != _bits(want)).nonzero()
    assert diff.numel() == 0, (gc.case_id(case), diff[:8].tolist(), [(float(got[r, c]), float(want[r, c])) for r, c in diff[:8].tolist()])
    again, _ = _run(dev, case, b)                                            # the same launch again: identical bits
    assert torch.equal(_bits(again), _bits(got))


def test_a_row_alone_equals_the_row_inside_a_batch(dev):
    case = dict(rows=5, V=25600, pad_c=8, pad_u=24, kind="ties", scale=3.0, alpha=0.1, ban=gc.BAN_FINITE, shared=False)
    b = gc.build(case, seed=5)
    full, _ = _run(dev, case, b)
    for r in range(5):
        one, _ = _run(dev, dict(case, rows=1), dict(cond=b["cond"][r:r + 1].clone(), uncond=b["uncond"][r:r + 1].clone(), whole=None))
        assert torch.equal(_bits(one[0]), _bits(full[r])), r
    order = torch.tensor([3, 0, 4, 1, 2])
    perm, _ = _run(dev, case, dict(cond=b["cond"][order].clone(), uncond=b["uncond"][order].clone(), whole=None))
    assert torch.equal(_bits(perm), _bits(full[order]))


def test_refusals_leave_the_logits_untouched(dev):
    import test_guidance_cpu as tcpu
    from youku_mplug_amd import _lib, ops
    g = torch.Generator().manual_seed(4)
    cond0 = torch.full((2, 72), gc.POISON, dtype=torch.bfloat16)
    cond0[:, :64] = torch.randn(2, 64, generator=g).to(torch.bfloat16)
    uncond0 = torch.randn(2, 64, generator=g).to(torch.bfloat16)
    (cond, cbuf), (uncond, ubuf) = _guarded(cond0, dev), _guarded(uncond0, dev)
    before = (cbuf.clone(), ubuf.clone())
    real = dict(cond=cond.data_ptr(), uncond=uncond.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib()
    for over in tcpu.REFUSALS:
        fields = dict(real)
        fields.update({k: (None if v is None else real[k] + (v & 15)) if k in real else v for k, v in over.items()})
        rc = lib.mpv_logits_guide(C.byref(tcpu._desc(**fields)), stream)
        torch.cuda.synchronize()
        assert rc < 0 and torch.equal(_bits(cbuf), _bits(before[0])) and torch.equal(_bits(ubuf), _bits(before[1])), over
    assert lib.mpv_logits_guide(C.byref(tcpu._desc(**real)), stream) == 0        # the accepted descriptor does edit
    torch.cuda.synchronize()
    assert not torch.equal(_bits(cbuf), _bits(before[0])) and torch.equal(_bits(ubuf), _bits(before[1]))
    for bad_c, bad_u, kw in ((cond.float(), uncond, {}), (cond, uncond.float(), {}), (cond, uncond[:1], {}), (cond.cpu(), uncond.cpu(), {}),
                             (cond, uncond, dict(alpha=1.5)), (cond, uncond, dict(alpha=-0.1)), (cond[:, ::2], uncond, {})):
        with pytest.raises(_lib.MpvError):
            ops.logits_guide(bad_c, bad_u, **dict(dict(scale=3.0), **kw))


# ------------------------------------------------------------------------------ on the tiny model
_MODEL = {}


def _caption_model(dev):
    if not _MODEL:
        import test_sampling_gpu as tg
        _MODEL["m"] = tg._caption_model(dev)
    return _MODEL["m"]


def _inputs(dev, B=3, Q=6, seed=8):
    """-> (query_embeds [B, Q, H], null features [Q, H], tokens [B, 5])"""
    from oracle.weights import CONFIG_TINY
    g = torch.Generator().manual_seed(seed)
    qe = (torch.randn(B + 1, Q, CONFIG_TINY.hidden, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    return qe[:B].contiguous(), qe[B].contiguous(), torch.randint(0, CONFIG_TINY.vocab, (B, 5), generator=g).to(dev)


@pytest.mark.parametrize("kv,weights,mixed", [("per_sequence", "bf16", False), ("shared_prefix", "bf16", False), ("shared_prefix", "bf16", True),
                                              ("shared_prefix", "fp8", False)])
def test_sample_batched_under_guidance_equals_the_loop_with_the_host_guide(dev, kv, weights, mixed):
    from youku_mplug_amd import generation, ops
    m, model, video, ids, mask = _caption_model(dev)
    td, eod = model.text_decoder, m["eod_id"]
    qe, null, tokens = _inputs(dev)
    guidance = generation.Guidance(3.0, 0.1, null)
    lens = [5, 2, 3]
    kw = dict(query_embeds=qe, prompt_length=lens if mixed else torch.tensor(lens, device=dev), termination_id=eod, temperature=1.2, num_samples=4,
              seed=9, mixed_prompts=mixed)
    names = generation.SAMPLER_OPS["ragged" if mixed else "uniform"]
    model.eval()
    with torch.no_grad():
        got, gsc = td.sample_batched(tokens.clone(), top_p=0.95, kv=kv, decode_weights=weights, guidance=guidance, return_scores=True, **kw)
        plain = td.sample_batched(tokens.clone(), top_p=0.95, kv=kv, decode_weights=weights, **kw)
        cfg = generation._gen_config(td)
        cfg.top_k, cfg.top_p = 0, 0.95
        make_state = generation.guided_state_fn(generation.make_state_fn(td, kv, weights), guidance, stg.on_host(), generation.BAN_SAMPLING)
        want, wsc = generation.sample_batched_loop(cfg, make_state, tokens.clone(), advance_fn=getattr(ops, names[0]), return_scores=True,
                                                   score_fn=getattr(ops, names[2]), **kw)
    assert torch.equal(got, want) and torch.equal(gsc.token_logprob, wsc.token_logprob) and torch.equal(gsc.sum_logprob, wsc.sum_logprob)
    assert torch.equal(gsc.count, wsc.count) and torch.isfinite(gsc.sum_logprob).all() and (gsc.sum_logprob <= 0).all()
    assert got.shape[0] == plain.shape[0] == 12
    for r in range(12):
        assert torch.equal(got[r, :lens[r // 4]], tokens[r // 4, :lens[r // 4]])


@pytest.mark.parametrize("kv,weights,groups,mixed", [("per_sequence", "bf16", 1, False), ("shared_prefix", "bf16", 1, False),
                                                     ("shared_prefix", "bf16", 2, False), ("shared_prefix", "bf16", 1, True),
                                                     ("shared_prefix", "fp8", 1, False)])
def test_beam_search_batched_under_guidance_equals_the_loop_with_the_host_guide(dev, kv, weights, groups, mixed):
    from youku_mplug_amd import generation, ops
    m, model, video, ids, mask = _caption_model(dev)
    td, eod = model.text_decoder, m["eod_id"]
    qe, null, tokens = _inputs(dev, seed=12)
    guidance = generation.Guidance(3.0, 0.0, null)
    gkw = dict(beam_groups=2, diversity_penalty=0.5) if groups == 2 else {}
    kw = dict(query_embeds=qe, beam_size=3, num_return_gen=2, stop_token=eod, prompt_length=[4, 2, 5] if mixed else 4, **gkw)
    model.eval()
    with torch.no_grad():
        got = td.beam_search_batched(tokens.clone(), kv=kv, decode_weights=weights, guidance=guidance, **kw)
        make_state = generation.guided_state_fn(generation.make_state_fn(td, kv, weights), guidance, stg.on_host(), generation.BAN_BEAM)
        want = generation.beam_search_batched_loop(generation._gen_config(td), make_state, tokens.clone(),
                                                   topk_fn=lambda lg, k, add: ops.logprob_topk(lg, k, add=add), advance_fn=ops.beam_advance,
                                                   **(dict(group_advance_fn=ops.beam_advance_groups) if groups == 2 else {}), **kw)
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert torch.equal(a.sequences, b.sequences) and torch.equal(a.scores, b.scores)
        assert a.sequences.shape[0] == 2 and torch.isfinite(a.scores).all()
        if groups == 2:
            assert torch.equal(a.group, b.group)


def test_caption_generate_under_guidance_equals_the_decoder_entry(dev):
    from youku_mplug_amd import generation
    m, model, video, ids, mask = _caption_model(dev)
    eod = m["eod_id"]
    sel = [0, 1, 0]
    text = types.SimpleNamespace(input_ids=ids[sel].to(dev), attention_mask=mask[sel].to(dev))
    pl = int(mask[0].sum()) - 1
    Q, H = model.num_learnable_token, model.text_width
    model.eval()
    with torch.no_grad():
        qf = model.encode_video(video[sel]).view(3, Q, H)
        zero = model.encode_video(torch.zeros((1,) + tuple(video.shape[1:]), dtype=video.dtype, device=dev))
        # the default null features are encode_video of the all-zero clip; given the same features the result is the decoder entry's
        res = model.generate(video[sel], text, termination_id=eod, batched=True, kv_cache="shared_prefix", beam_size=3, num_return_gen=2, guidance_scale=3.0)
        given = model.generate(video[sel], text, termination_id=eod, batched=True, kv_cache="shared_prefix", beam_size=3, num_return_gen=2, guidance_scale=3.0,
                               guidance_query_features=zero)
        want = model.text_decoder.beam_search_batched(text.input_ids, query_embeds=qf.contiguous(), beam_size=3, num_return_gen=2, stop_token=eod,
                                                      prompt_length=pl, kv="shared_prefix", guidance=generation.Guidance(3.0, 0.0, zero))
        plain = model.generate(video[sel], text, termination_id=eod, batched=True, kv_cache="shared_prefix", beam_size=3, num_return_gen=2)
        for i in range(3):
            assert torch.equal(res[i], want[i].sequences.cpu()) and torch.equal(given[i], res[i])
        assert torch.equal(res[0], res[2]) and len(plain) == 3
        smp, sc = model.generate(video[sel], text, termination_id=eod, do_sample=True, num_samples=3, seed=31, guidance_scale=3.0, guidance_alpha=0.1,
                                 guidance_query_features=zero.repeat(3, 1), return_scores=True)
        streams = torch.arange(9, device=dev)
        toks, wsc = model.text_decoder.sample_batched(text.input_ids, query_embeds=qf.contiguous(), num_samples=3, seed=31, streams=streams,
                                                      termination_id=eod, prompt_length=torch.full((3,), pl, device=dev), return_scores=True,
                                                      guidance=generation.Guidance(3.0, 0.1, zero))
        width = smp[0].shape[1]
        padded = generation.pad_after_termination(toks, pl, eod, width, eod).cpu()
        for i in range(3):
            assert torch.equal(smp[i], padded[3 * i:3 * i + 3]) and torch.equal(sc[i]["sum_logprob"], wsc.sum_logprob[3 * i:3 * i + 3].cpu())
    with pytest.raises(ValueError, match="batched=True or do_sample=True"):
        model.generate(video[sel], text, termination_id=eod, guidance_scale=3.0)
