"""Beam search with the finished clips' slots refilled in flight, on one GPU: the decoder, the constants and the method of
tools/bench_sample_inflight.py (the 1.3B dims with synthetic weights, 256 query slots, kv="shared_prefix"), 128 clips with 8-token
prompts through 32 slots x 5 beams (160 resident sequences), the stop token BANNED on both paths (banned_token_ids: a random-weight
decoder would close no hypothesis store in any case), so that a clip's length is its BUDGET: the budgets cycle over BUDGETS (6 .. 30
positions), as captions of different lengths would end; a second case gives every clip the same budget of 18.

  lockstep   the path before the in-flight loop: beam_search_batched(kv="shared_prefix") on chunks of 32 clips in input order, every
             chunk run to its longest budget (tokens_to_generate = that budget), as generate(batched=True) holds a chunk until its
             slowest clip is done;
  inflight   beam_search_inflight on all 128 clips with 32 slots and the clips' own budgets, for several refill_min.

    python tools/bench_beam_inflight.py [--out profiles/beam_inflight.json] [--rounds 3] [--refill_min 1 4 8 16]

Times are host clocks around calls that end in the download of the search state (a device synchronise precedes and follows); every
path runs once before the timed rounds and the paths alternate inside a round; decode steps and prefill passes are counted and written
next to the times.  No ratio is promised: the JSON holds medians, run-to-run spreads and the step counts.  (The best sequences of the
two paths are compared on the columns up to the clip's own budget and counted, not asserted: the lockstep chunk searches every clip on
to the chunk's longest budget, and the best beam of a longer search need not extend the best beam at the clip's budget; with equal
budgets the two searches are the same.)"""
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
from bench_sample_inflight import BUDGETS, CLIPS, EQUAL, PROMPT, SLOTS  # noqa: E402

BEAMS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_inflight.json"))
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
    ban = generation.LogitsConstraints(banned_token_ids=(base.STOP,))
    rec = {"decoder": dict(hidden=base.HIDDEN, layers=base.LAYERS, heads=base.HEADS, ffn=base.FFN, vocab=base.VOCAB), "query_slots": base.Q,
           "clips": CLIPS, "slots": SLOTS, "beams": BEAMS, "resident_rows": SLOTS * BEAMS, "prompt_tokens": PROMPT, "budget_cycle": BUDGETS,
           "equal_budget": EQUAL, "rounds": args.rounds, "stop_token": "banned", "device": torch.cuda.get_device_name(0), "cases": {}}
    with torch.no_grad():
        qe = (torch.randn(CLIPS, base.Q, base.HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
        tokens = torch.randint(8, base.VOCAB, (CLIPS, PROMPT), generator=gen).to(dev)
        lens = [PROMPT] * CLIPS
        for which, budgets in (("budgets_6_30", [BUDGETS[c % len(BUDGETS)] for c in range(CLIPS)]), ("equal_budgets", [EQUAL] * CLIPS)):
            kw = dict(beam_size=BEAMS, num_return_gen=1, stop_token=base.STOP, constraints=ban)
            last, seen = {}, {}

            def lockstep():
                rows = []
                counts.update(steps=0, prefills=0)
                for c0 in range(0, CLIPS, SLOTS):
                    sel = list(range(c0, c0 + SLOTS))
                    gpt.config.extra["tokens_to_generate"] = max(budgets[c] for c in sel)          # the chunk runs to its longest budget
                    outs = gpt.beam_search_batched(tokens[sel], query_embeds=qe[sel].contiguous(), prompt_length=PROMPT, kv="shared_prefix", **kw)
                    rows += [o.sequences[0].cpu() for o in outs]
                gpt.config.extra["tokens_to_generate"] = max(BUDGETS)
                last["lockstep"] = rows
                seen["lockstep"] = dict(decode_steps=counts["steps"], prefills=counts["prefills"])

            def make_inflight(rm):
                def run():
                    counts.update(steps=0, prefills=0)
                    out = gpt.beam_search_inflight(tokens, query_embeds=qe, prompt_length=lens, slots=SLOTS, max_new_tokens=budgets, refill_min=rm, **kw)
                    last[run.__name__] = [o.sequences[0].cpu() for o in out.results]
                    seen[run.__name__] = dict(decode_steps=out.steps, prefills=out.prefills, staged_prefill_calls=counts["prefills"])
                run.__name__ = f"inflight_refill{rm}"
                return run
            fns = [lockstep] + [make_inflight(rm) for rm in args.refill_min]
            times = timed(fns, args.rounds)
            med, spread = summary(times)
            equal = {}
            for fn in fns[1:]:
                n_eq = 0
                for c in range(CLIPS):
                    w = PROMPT + budgets[c]
                    n_eq += int(torch.equal(last[fn.__name__][c][:w], last["lockstep"][c][:w]))
                equal[fn.__name__] = n_eq
            base_noise = spread["lockstep"] * med["lockstep"]
            rec["cases"][which] = dict(
                seconds=times, median_s=med, run_to_run_spread=spread, launches=seen, best_sequences_equal_to_lockstep=equal,
                lockstep_spread_s=base_noise, inflight_over_lockstep={k: med[k] / med["lockstep"] for k in med if k != "lockstep"},
                inflight_minus_lockstep_s={k: med[k] - med["lockstep"] for k in med if k != "lockstep"},
                beyond_lockstep_spread={k: bool(abs(med[k] - med["lockstep"]) > base_noise) for k in med if k != "lockstep"})
            line = "  ".join(f"{k} {med[k]:.4f} s ({spread[k]:.1%}; {seen[k]['decode_steps']} steps, {seen[k]['prefills']} prefills; "
                             f"{equal.get(k, CLIPS)}/{CLIPS} clips equal)" for k in med)
            print(f"[{which}] {line}", flush=True)
    generation.SharedPrefixDecodeState.step, generation.SharedPrefixDecodeState.prefill_fan_out = step, prefill
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
