"""Sampled captions with the finished clips' slots refilled in flight, on one GPU: the decoder and the constants of
tools/bench_mixed_sampling.py (the 1.3B dims with synthetic weights, 256 query slots, kv="shared_prefix", top-p 0.9), 128 clips with
8-token prompts through 32 slots, termination banned (a random-weight decoder would not terminate in any case; termination id -1), so
that a clip's length is its BUDGET: the budgets cycle over BUDGETS (6 .. 30 tokens), as captions of different lengths would end.

  lockstep   the path before the in-flight loop: sample_batched(mixed_prompts=True) on chunks of 32 clips in input order, every chunk
             run to its longest budget (tokens_to_generate = that budget), as generate(sample_mixed_prompts=True) holds a chunk until
             its slowest caption ends;
  inflight   sample_inflight on all 128 clips with 32 slots and the clips' own budgets, for several refill_min.

Both at 16 samples per clip (512 resident rows) and at 1 greedy sample (top_k = 1, 32 rows), and once more with EQUAL budgets, where the
in-flight loop has nothing to gain and pays for its scatter launches and staged prefills.

    python tools/bench_sample_inflight.py [--out profiles/sample_inflight.json] [--rounds 3] [--refill_min 1 4 8 16]

Times are host clocks around calls that end in a download of the token table (a device synchronise precedes and follows); every path
runs once before the timed rounds and the paths alternate inside a round; decode steps and prefill passes are counted and written next
to the times.  No ratio is promised: the JSON holds medians, run-to-run spreads and the step counts."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_caption_batched as base  # noqa: E402  (the decoder's dims and the constants of the caption benchmark)
from bench_mixed_prompts import summary, timed  # noqa: E402

CLIPS, SLOTS, PROMPT, TOP_P = 128, 32, base.PROMPT, 0.9
BUDGETS = [6, 30, 12, 18, 24, 9, 27, 15, 21, 7, 10, 28, 14, 20, 8, 26]          # 16 budgets, mean 17.2: clip c gets BUDGETS[c % 16]
EQUAL = 18


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_inflight.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--refill_min", type=int, nargs="+", default=[1, 4, 8, 16])
    args = ap.parse_args()
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import generation
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    dev = torch.device("cuda:0")
    cfg = GPT3Config(vocab_size=base.VOCAB, hidden_size=base.HIDDEN, ffn_hidden_size=base.FFN, num_hidden_layers=base.LAYERS,
                     num_attention_heads=base.HEADS, max_position_embeddings=base.MAX_POS, layernorm_epsilon=base.LN_EPS,
                     tokens_to_generate=max(BUDGETS), eod_id=base.STOP)
    torch.manual_seed(0)
    gpt = DistributedGPT3(config=cfg, device=dev).eval()
    counts = {"steps": 0, "prefills": 0}
    step, prefill = generation.SharedPrefixDecodeState.step, generation.SharedPrefixDecodeState.prefill_fan_out

    def counted_step(self, *a, **k):
        counts["steps"] += 1
        return step(self, *a, **k)

    def counted_prefill(self, tokens, query_embeds, fan, prompt_len=None):      # (the loops look for the prompt_len parameter)
        counts["prefills"] += 1
        return prefill(self, tokens, query_embeds, fan, prompt_len=prompt_len)
    generation.SharedPrefixDecodeState.step, generation.SharedPrefixDecodeState.prefill_fan_out = counted_step, counted_prefill
    gen = torch.Generator().manual_seed(1)
    rec = {"decoder": dict(hidden=base.HIDDEN, layers=base.LAYERS, heads=base.HEADS, ffn=base.FFN, vocab=base.VOCAB), "query_slots": base.Q,
           "clips": CLIPS, "slots": SLOTS, "prompt_tokens": PROMPT, "top_p": TOP_P, "budget_cycle": BUDGETS, "equal_budget": EQUAL,
           "rounds": args.rounds, "termination": "banned", "device": torch.cuda.get_device_name(0), "cases": {}}
    with torch.no_grad():
        qe = (torch.randn(CLIPS, base.Q, base.HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
        tokens = torch.randint(8, base.VOCAB, (CLIPS, PROMPT), generator=gen).to(dev)
        lens = [PROMPT] * CLIPS
        for name, samples, sampler in (("samples16", 16, dict(top_p=TOP_P, top_k=0)), ("greedy1", 1, dict(top_k=1, top_p=0.0))):
            for which, budgets in (("budgets_6_30", [BUDGETS[c % len(BUDGETS)] for c in range(CLIPS)]), ("equal_budgets", [EQUAL] * CLIPS)):
                kw = dict(num_samples=samples, seed=5, temperature=1.0, termination_id=-1, **sampler)
                last, seen = {}, {}

                def lockstep():
                    rows = []
                    counts.update(steps=0, prefills=0)
                    for c0 in range(0, CLIPS, SLOTS):
                        sel = list(range(c0, c0 + SLOTS))
                        gpt.config.extra["tokens_to_generate"] = max(budgets[c] for c in sel)      # the chunk runs to its longest budget
                        streams = (torch.as_tensor(sel)[:, None] * samples + torch.arange(samples)[None]).reshape(-1)
                        rows.append(gpt.sample_batched(tokens[sel], query_embeds=qe[sel].contiguous(), streams=streams, prompt_length=lens[:SLOTS],
                                                       mixed_prompts=True, kv="shared_prefix", use_eod_token_for_early_termination=False, **kw).cpu())
                    gpt.config.extra["tokens_to_generate"] = max(BUDGETS)
                    last["lockstep"] = rows
                    seen["lockstep"] = dict(decode_steps=counts["steps"], prefills=counts["prefills"])

                def make_inflight(rm):
                    def run():
                        counts.update(steps=0, prefills=0)
                        out = gpt.sample_inflight(tokens, query_embeds=qe, prompt_length=lens, slots=SLOTS, max_new_tokens=budgets, refill_min=rm, **kw)
                        last[run.__name__] = out.tokens.cpu()
                        seen[run.__name__] = dict(decode_steps=out.steps, prefills=out.prefills, staged_prefill_calls=counts["prefills"])
                    run.__name__ = f"inflight_refill{rm}"
                    return run
                fns = [lockstep] + [make_inflight(rm) for rm in args.refill_min]
                times = timed(fns, args.rounds)
                med, spread = summary(times)
                # the two paths' tokens on the columns both wrote (the greedy rows are expected to agree wherever the logits' last digit
                # does not flip an arg-max; sampled rows of 32-row-count-equal steps too; counted, not asserted)
                equal = {}
                for fn in fns[1:]:
                    got, n_eq = last[fn.__name__], 0
                    for c in range(CLIPS):
                        want = last["lockstep"][c // SLOTS][(c % SLOTS) * samples:(c % SLOTS + 1) * samples]
                        w = min(PROMPT + budgets[c], want.shape[1])
                        n_eq += int(torch.equal(got[c * samples:(c + 1) * samples, :w], want[:, :w]))
                    equal[fn.__name__] = n_eq
                base_noise = spread["lockstep"] * med["lockstep"]
                rec["cases"][f"{name}_{which}"] = dict(
                    samples_per_clip=samples, resident_rows=SLOTS * samples, seconds=times, median_s=med, run_to_run_spread=spread, launches=seen,
                    clips_equal_to_lockstep=equal, lockstep_spread_s=base_noise,
                    inflight_minus_lockstep_s={k: med[k] - med["lockstep"] for k in med if k != "lockstep"},
                    beyond_lockstep_spread={k: bool(abs(med[k] - med["lockstep"]) > base_noise) for k in med if k != "lockstep"})
                line = "  ".join(f"{k} {med[k]:.4f} s ({spread[k]:.1%}; {seen[k]['decode_steps']} steps, {seen[k]['prefills']} prefills; "
                                 f"{equal.get(k, CLIPS)}/{CLIPS} clips equal)" for k in med)
                print(f"[{name} {which}] {line}", flush=True)
    generation.SharedPrefixDecodeState.step, generation.SharedPrefixDecodeState.prefill_fan_out = step, prefill
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
