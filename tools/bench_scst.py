"""Cost of the self-critical training step's reward on one GPU, written to profiles/scst.json.  The decoder and
the constants are those of tools/bench_consensus.py: the 1.3B dims with synthetic weights, 256 query slots, 8-token prompts, 16 samples
per clip; 32 clips and 5 references per clip; captions of 30 and of 100 tokens.

  1. kernel     ops.caption_cider alone: 32 x 16 candidate rows against 32 x 5 reference rows (2 560 pairs), ids over a 64-token
                alphabet (n-grams of every order hit, and most are in the corpus table) and random ids over the vocabulary (nothing
                hits: every probe ends at an empty slot).  HIP events around 20 calls after 3 warm-up ones; the wrapper's one small
                upload of the starts and offsets is inside.
  2. host       the fp64 dict restatement of the tests (tests/ref_cider.py) on the same input, wall clock, once: for context only, it
                is no gate -- what a host scorer would put on the step's path, before the device-to-host-to-device round trip.
  3. step       DistributedGPT3_Caption.forward_scst + backward on a model with the 1.3B decoder (frozen) and the tiny ViT, in train
                mode: the rollout (sampler), the reward (the references' upload and the ops.caption_cider call) and the rest (encode,
                training forward + backward over clips x samples sequences), each between device synchronisations.  A random-weight
                decoder almost never draws the termination id, so nearly every sample is max_new_tokens long.  The training pass keeps the activations of
                clips x samples sequences: when 32 clips do not fit -- the card's memory, or the 2 GiB operand limit of the GEMM entry (the MLP's
                [sequences x positions, 8192] activation, the window's logits), which forward_scst refuses before any launch -- the
                step is measured at the largest halving that does, and the record
                says which and why.

    python tools/bench_scst.py [--out profiles/scst.json] [--rounds 3]

No number is promised and no caption-quality claim is made: there is no trained checkpoint and no data set behind these figures."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "tests")]

import bench_caption_batched as base  # noqa: E402  (the decoder's dims and the constants of the caption benchmark)

CLIPS, SAMPLES, REFS, PROMPT = 32, 16, 5, base.PROMPT
LENGTHS = (30, 100)
TERM = base.STOP


def tables(length, high, gen):
    cands = torch.randint(8, high, (CLIPS * SAMPLES, PROMPT + length), generator=gen)
    refs = torch.randint(8, high, (CLIPS * REFS, length), generator=gen)
    return cands, refs


def kernel_rows(dev):
    import ref_cider as rc
    from youku_mplug_amd import generation, ops
    out = []
    gen = torch.Generator().manual_seed(3)
    for length in LENGTHS:
        for content, high in (("alphabet_64", 72), ("random_ids", base.VOCAB)):
            cands, refs = tables(length, high, gen)
            start_a, begin_a = [PROMPT] * (CLIPS * SAMPLES), list(range(0, CLIPS * SAMPLES + 1, SAMPLES))
            start_b, begin_b = [0] * (CLIPS * REFS), list(range(0, CLIPS * REFS + 1, REFS))
            t0 = time.perf_counter()
            stats = generation.CiderStats.from_token_table(refs, start_b, begin_b, -1, base.VOCAB)
            build_s = time.perf_counter() - t0
            ca, rb = cands.to(dev), refs.to(dev)
            stats.arrays(dev)
            call = lambda: ops.caption_cider(ca, start_a, begin_a, rb, start_b, begin_b, term=-1, stats=stats)
            for _ in range(3):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(20):
                pair, score = call()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / 20
            # the host restatement on the same input, once
            rows_a, rows_b = [r[PROMPT:] for r in cands.tolist()], refs.tolist()
            t0 = time.perf_counter()
            df, log_ref_len = rc.doc_freq([rows_b[c * REFS:(c + 1) * REFS] for c in range(CLIPS)])
            want = [rc.score_of([rc.pair_values(rows_a[c * SAMPLES + s], r, df, log_ref_len) for r in rows_b[c * REFS:(c + 1) * REFS]])
                    for c in range(CLIPS) for s in range(SAMPLES)]
            host_s = time.perf_counter() - t0
            err = max(abs(g - w) / max(abs(w), 1e-300) if w else abs(g) for g, w in zip(score.tolist(), want))
            assert err <= 1e-12, err
            out.append(dict(clips=CLIPS, samples=SAMPLES, references=REFS, pairs=int(pair.shape[0]), caption_tokens=length, content=content,
                            corpus_entries=stats.entries, table_slots=stats.capacity, stats_build_host_s=round(build_s, 4),
                            call_us=round(us, 1), host_restatement_s=round(host_s, 4), host_over_device=round(host_s / (us * 1e-6), 1),
                            mean_score=round(sum(want) / len(want), 4), worst_relative_difference=err,
                            note="wrapper included: one small upload of the starts and offsets per call; the host figure is context, no gate"))
            print(f"kernel: {length:3d} tokens, {content:12s}: {us:9.1f} us per call; host restatement {host_s:.3f} s", flush=True)
    return out


def step_rows(dev, rounds):
    from oracle.weights import CONFIG_TINY
    from youku_mplug_amd import generation, ops
    from youku_mplug_amd.downstream import synthetic_gencls_model
    shapes = dataclasses.replace(CONFIG_TINY, hidden=base.HIDDEN, layers=base.LAYERS, heads=base.HEADS, ffn=base.FFN, vocab=base.VOCAB,
                                 max_pos=base.MAX_POS, num_queries=base.Q, gpt_ln_eps=base.LN_EPS)
    torch.manual_seed(0)
    model = synthetic_gencls_model(shapes, "caption", device=dev).train()
    gen = torch.Generator().manual_seed(1)
    spent, limits = {}, []

    def clocked(name, fn):
        def run(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            spent[name] = spent.get(name, 0.0) + time.perf_counter() - t0
            return out
        return run
    model._scst_rollout = clocked("rollout", model._scst_rollout)
    plain_cider = ops.caption_cider
    out = []
    for length in LENGTHS:
        clips = CLIPS
        while clips >= 1:
            video = torch.randn((clips, 3, CONFIG_TINY.num_frames, CONFIG_TINY.img_size, CONFIG_TINY.img_size), generator=gen).to(dev).to(torch.bfloat16)
            ids = torch.randint(8, base.VOCAB, (clips, PROMPT + 1), generator=gen).to(dev)
            text = types.SimpleNamespace(input_ids=ids, attention_mask=torch.ones_like(ids))
            refs = [[r for r in torch.randint(8, 72, (REFS, length), generator=gen).tolist()] for _ in range(clips)]
            stats = generation.CiderStats(refs, base.VOCAB)
            times = []
            try:
                for it in range(rounds + 1):                                     # the first round warms up and is dropped
                    spent.clear()
                    ops.caption_cider = clocked("reward_call", plain_cider)
                    model.zero_grad(set_to_none=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    loss, st = model.forward_scst(video, text, refs, cider=stats, num_samples=SAMPLES, top_p=0.9, seed=5 + it, max_new_tokens=length,
                                                  termination_id=TERM)
                    loss.backward()
                    torch.cuda.synchronize()
                    total = time.perf_counter() - t0
                    if it:
                        times.append(dict(total=total, rollout=spent["rollout"], reward_call=spent["reward_call"],
                                          rest=total - spent["rollout"] - spent["reward_call"]))
                break
            except (torch.cuda.OutOfMemoryError, ValueError) as e:      # forward_scst refuses a pass beyond the operand limit before any launch
                if isinstance(e, ValueError) and "larger than 2 GiB" not in str(e):
                    raise
                why = "the card's memory" if isinstance(e, torch.cuda.OutOfMemoryError) else "the GEMM entry's 2 GiB operand limit"
                limits.append(dict(clips=clips, caption_tokens=length, exceeds=why))
                print(f"step: {clips} clips x {SAMPLES} samples at {length} tokens exceed {why}: halving", flush=True)
                del video, ids, text
                model.zero_grad(set_to_none=True)
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                clips //= 2
            finally:
                ops.caption_cider = plain_cider
        med = {k: statistics.median(t[k] for t in times) for k in times[0]}
        out.append(dict(clips=clips, clips_asked=CLIPS, samples=SAMPLES, references=REFS, caption_tokens=length, rounds=rounds,
                        sequence_positions=base.Q + PROMPT + length, seconds=[{k: round(v, 4) for k, v in t.items()} for t in times],
                        median_s={k: round(v, 4) for k, v in med.items()}, reward_share_of_step=round(med["reward_call"] / med["total"], 5),
                        mean_sampled_tokens=st["length"], did_not_fit=[x for x in limits if x["caption_tokens"] == length], peak_memory_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
                        note="reward_call: ops.caption_cider with its upload, between synchronisations (it overstates the call: in the step "
                             "nothing waits for it); rest: encode, the references' upload, the training forward + backward"))
        print(f"step: {clips} clips, {length:3d} tokens: total {med['total']:.3f} s = rollout {med['rollout']:.3f} + reward {med['reward_call']:.4f} "
              f"+ rest {med['rest']:.3f}", flush=True)
        torch.cuda.reset_peak_memory_stats()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scst.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip_step", action="store_true", help="the kernel and host figures only")
    args = ap.parse_args()
    import youku_mplug_amd  # noqa: F401
    dev = torch.device("cuda:0")
    rec = {"decoder": dict(hidden=base.HIDDEN, layers=base.LAYERS, heads=base.HEADS, ffn=base.FFN, vocab=base.VOCAB), "query_slots": base.Q,
           "clips": CLIPS, "samples_per_clip": SAMPLES, "references_per_clip": REFS, "prompt_tokens": PROMPT, "termination": "id 7, almost never drawn (random weights)",
           "device": torch.cuda.get_device_name(0), "clock": "HIP events (kernel), host perf_counter between synchronisations (step, host)"}
    with torch.no_grad():
        rec["kernel"] = kernel_rows(dev)
    if not args.skip_step:
        rec["step"] = step_rows(dev, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
