"""Video captioning fine-tuning / evaluation on the MI355X-native path -- drop-in for the reference's
downstream/run_caption_distributed_gpt3.py (same command line, YAML / JSON configs, per-step protocol, result files), with
DistributedGPT3_Caption (caption loss; beam search over the KV-cache decode path) and the engine coming from youku_mplug_amd
(SURVEY.md section 8(f) ranks 1 and 3).

What this entry point adds to downstream/finetune_common.py:
  * the training batch (:113-115): [config["prompt"], caption] pairs padded to max_length, prompt masked out of the loss;
    `model(video, text)` -> loss_generation;
  * evaluation (:208-238): the prompt alone (padded to 20 tokens) + the clip's query features -> `model.generate` (one beam search
    per clip), decoded, blanks removed, the prompt cut off -> [{video_id, pred_caption, gold_caption}];
  * `--eval_batched_beam` (not in the reference, default off): `model.generate(..., batched=True)` searches the clips of a batch in
    lockstep (`--clips_per_search` at a time, generation.beam_search_batched_loop); same result files;
  * `--eval_sample N` (not in the reference, default off): N sampled captions per clip next to the beam caption, as
    "sampled_captions" in the result file (`model.generate(..., do_sample=True, num_samples=N)`: the sampler on the device);
  * `--eval_shared_kv` (not in the reference, default off): `--eval_batched_beam` and `--eval_sample` cache the query slots and the
    prompt once per clip instead of once per beam or sample (`model.generate(..., kv_cache="shared_prefix")`); same result files;
  * `--eval_repetition_penalty F`, `--eval_no_repeat_ngram N`, `--eval_min_new_tokens N` (not in the reference, defaults off): the
    `--eval_batched_beam` and `--eval_sample` calls penalise repeated tokens, never repeat an n-gram of N tokens and do not end a
    caption before N tokens, on the device (`model.generate(..., repetition_penalty=F, no_repeat_ngram_size=N, min_new_tokens=N)`);
    without one of those two flags (or `--eval_sample_best_of`) they are an error;
  * `--eval_sample_best_of N` (not in the reference, default 0 = off): the caption of a clip is the most likely of N sampled ones
    instead of the beam search's (`model.generate(..., do_sample=True, num_samples=N, best_of=True)`: the model's log-probability per
    token, recorded on the device while sampling), written as "pred_caption" through the same result path, so the metrics below run
    on it; it combines with `--eval_shared_kv` and the constraint flags;
  * `--eval_beam_groups G` with `--eval_diversity_penalty F` (not in the reference, default 1 = off): diverse (group) beam search in
    lockstep, G groups of min(5, 16 // G) beams each, a later group penalised by F for every token an earlier group chose at the same
    step (`model.generate(..., batched=True, beam_groups=G, diversity_penalty=F, rerank_by_logprob=True)`); every hypothesis of every
    group is re-scored by the model's own log-probability per token: "pred_caption" is the best, "pred_candidates" lists all of them in
    that order; it implies the batched path and combines with `--eval_shared_kv` and the constraint flags;
  * `--eval_fp8_decode` (not in the reference, default off): every generation call of the evaluation runs its decode steps on e4m3
    codes of the decoder's weights (`model.generate(..., decode_weights="fp8")`: quantised on the device, once; the bf16 weights stay
    and serve the prefill of many rows and the scoring); it combines with every other flag;
  * `--eval_mixed_prompts` (not in the reference, default off; implies nothing else): the lockstep beam searches (`--eval_batched_beam`,
    `--eval_beam_groups`) take the clips of a batch in input order, `--clips_per_search` at a time, whatever their prompt lengths,
    instead of one search per distinct length (`model.generate(..., mixed_prompts=True)`; needs `--eval_shared_kv`); same result files;
  * `--eval_sample_mixed_prompts` (not in the reference, default off; implies nothing else): the sampling calls (`--eval_sample`,
    `--eval_sample_best_of`) take the clips of a batch in input order, `--clips_per_search` at a time, whatever their prompt lengths,
    instead of one lockstep loop per distinct length (`model.generate(..., do_sample=True, sample_mixed_prompts=True)`; needs one of
    those two flags and `--eval_shared_kv`); the beam-search calls are not touched; same result files;
  * `--eval_sample_inflight` (not in the reference, default off; implies nothing else): the sampling calls (`--eval_sample`,
    `--eval_sample_best_of`) run ONE loop over all the clips of a batch in which `--clips_per_search` clips stay resident and a finished
    clip's rows go to the next clip while the others continue (`model.generate(..., do_sample=True, inflight=True)`: continuous
    batching; needs one of those two flags and `--eval_shared_kv`; it replaces `--eval_sample_mixed_prompts`, which it is refused
    with); the beam-search calls are not touched; same result files;
  * `--eval_beam_inflight` (not in the reference, default off; implies nothing else): the lockstep beam search (`--eval_batched_beam`,
    with or without `--eval_beam_groups`) runs ONE loop over all the clips of a batch in which `--clips_per_search` clips stay resident
    and a finished clip's beams go to the next clip while the others continue (`model.generate(..., batched=True, beam_inflight=True)`;
    needs `--eval_batched_beam` and `--eval_shared_kv`; refused with `--eval_mixed_prompts` and with the sampling flags); same result
    files;
  * `--eval_allowed_phrases FILE` (not in the reference, default off): a closed vocabulary, one phrase per line (blank lines are
    skipped).  The lockstep beam search is constrained to the trie of the phrases (`model.generate(..., batched=True,
    allowed_phrases=)`: one mask launch per step, a cost that does not grow with the number of phrases): "pred_caption" is the best
    phrase, "pred_candidates" lists the up to 5 best as {"caption", "phrase_index", "score"}, the score renormalised over the allowed
    tokens; needs `--eval_batched_beam`, combines with `--eval_shared_kv`, `--eval_fp8_decode`, `--eval_mixed_prompts` and
    `--eval_beam_inflight`, and is refused with `--eval_beam_groups`, `--eval_sample_best_of` and `--eval_min_new_tokens`;
  * `--eval_sample_consensus N` with `--eval_consensus_metric rouge_l|ngram_f` (not in the reference, default 0 = off): the caption of
    a clip is the CONSENSUS (minimum-Bayes-risk) choice among N sampled ones instead of the beam search's -- the sample with the
    largest mean ROUGE-L (beta 1.2; the default) or mean clipped-n-gram F against all N samples, counted over token ids on the device
    (`model.generate(..., do_sample=True, num_samples=N, consensus=METRIC)`); the chosen caption goes through the result path and the
    metrics above like `--eval_sample_best_of`'s, with which (as with `--eval_beam_groups` and `--eval_allowed_phrases`) it is
    refused; it combines with `--eval_shared_kv`, the constraints, `--eval_sample_mixed_prompts` and `--eval_sample_inflight`;
  * `--eval_guidance_scale F` with `--eval_guidance_alpha F` (not in the reference, defaults 1.0 / 0.0 = off): the lockstep generation
    calls of the evaluation are GUIDED (classifier-free guidance / contrastive decoding): every chunk decodes a second branch of the
    same prompts behind the query features of an all-zero clip and each step continues from cond + (scale - 1) * (cond - uncond)
    (`model.generate(..., guidance_scale=F)`; one more launch per step, twice the rows per chunk); the alpha -- a token below alpha
    times the step's most likely one is banned -- acts on the sampling calls only (`guidance_alpha=F`; the beam search refuses it).
    Needs one of the lockstep flags (`--eval_batched_beam`, `--eval_beam_groups`, `--eval_sample`, `--eval_sample_best_of`,
    `--eval_sample_consensus`), is refused with `--eval_sample_inflight` and `--eval_beam_inflight`, and combines with the rest;
  * `--eval_score_gold` (not in the reference, default off): evaluation also scores every clip's `gold_caption` list, teacher-forced,
    against the query features computed once for that clip (`model.score_captions(..., query_features=)`: one packed pass per batch,
    no padding rows), adds "gold_logprob" / "gold_tokens" lists to the result entries and logs the corpus per-token NLL and perplexity;
    it combines with every flag above, and without it the run is the one described above;
  * `--scst` with `--scst_samples N`, `--scst_baseline mean_others|greedy`, `--scst_temperature F` and `--scst_stats FILE` (not in the
    reference, all off by default: without `--scst` the loop is the one above): self-critical sequence training -- a step samples N
    captions per clip from the model, rewards each with CIDEr over token ids against the clip's own caption(s) on the device and
    weights its log-likelihood by reward minus baseline (`model.forward_scst`).  The corpus statistics are a
    saved `generation.CiderStats` (FILE) or, by default, built at start-up from the training set's captions (with
    `--synthetic_steps`, the synthetic ones); a step is one `forward_scst` call, and a batch whose prompts differ in length (the
    tokenizer shortens the prompt of an over-long pair) is refused.  `--scst_shared_prefix` (needs `--scst`, default off) runs the
    step's training pass on a shared prefix, as the rollout already runs: every clip's query slots and prompt once, its samples as
    packed continuations (`forward_scst(training_pass="shared_prefix")`; that pass applies no decoder dropout);
  * corpus CIDEr in the evaluation's result dict ("CIDEr": the mean over clips of the scorer's 10 x mean-over-orders score): over the
    same CJK-character units as BLEU / ROUGE-L, the units mapped to ids in order of first appearance, df from this evaluation's own
    references as the reference project's scorer takes it, ONE `ops.caption_cider` call (`corpus_cider`).  Past 65 535 distinct
    units, with a caption of more than 255 units, or on a CPU run it is left out and the log line says so;
  * save_result (dataset/utils.py:114-160): one JSON per rank, merged by rank 0; cal_metric (:240-298): predictions and references
    reduced to their CJK characters, one token per character, scored by pycocoevalcap's COCOEvalCap when that package is importable.
    It is not on this image: then BLEU-1..4 (corpus level, closest-reference brevity penalty) and ROUGE-L (beta 1.2, best reference)
    are computed here as that package defines them, CIDEr on the device (above), and METEOR is left out -- said in the log line,
    not guessed;
  * main (:418-440, 446-470): `--evaluate_only` scores the validation split and writes one log line; training epochs do not
    evaluate (the reference has that block commented out)."""
import argparse
import json
import math
import os
import re
import sys
from collections import Counter

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import finetune_common as ft  # noqa: E402
from youku_mplug_amd.downstream import DistributedGPT3_Caption  # noqa: E402


def make_training_batch(video, text, prompt, tokenizer, device, max_length):
    input_text = [[prompt, x] for x in text]
    text_input = tokenizer(input_text, padding="max_length", truncation=True, max_length=max_length, return_tensors="pt").to(device)
    return video.to(device, non_blocking=True).bfloat16(), text_input


@torch.no_grad()
def evaluation(model, data_loader, tokenizer, device, config, batched=False, clips_per_search=32, eval_sample=0, seed=0, shared_kv=False,
               constraints=None, best_of=0, score_gold=False, max_length=None, beam_groups=1, diversity_penalty=0.0, fp8_decode=False,
               mixed_prompts=False, sample_mixed_prompts=False, sample_inflight=False, beam_inflight=False, allowed_phrases=None,
               consensus=0, consensus_metric="rouge_l", guidance_scale=1.0, guidance_alpha=0.0):
    """-> [{video_id, pred_caption, gold_caption}] (:208-238); batched: `--eval_batched_beam`; eval_sample: `--eval_sample`;
    shared_kv: `--eval_shared_kv`, constraints: the keywords of `--eval_repetition_penalty` / `--eval_no_repeat_ngram` /
    `--eval_min_new_tokens` (the lockstep calls only); best_of: `--eval_sample_best_of` (the prediction is the best of that many
    samples instead of the beam search's); score_gold: `--eval_score_gold` (the clip's query features are computed once and serve the
    generation and the scoring of its gold captions, tokenized as the training pairs are, at most max_length tokens); beam_groups /
    diversity_penalty: `--eval_beam_groups` / `--eval_diversity_penalty` (the prediction is the most likely hypothesis of a diverse beam
    search, all of them in "pred_candidates"); fp8_decode: `--eval_fp8_decode`; mixed_prompts: `--eval_mixed_prompts` (the
    lockstep beam-search calls only); sample_mixed_prompts: `--eval_sample_mixed_prompts` (the sampling calls only); sample_inflight:
    `--eval_sample_inflight` (the sampling calls only); beam_inflight: `--eval_beam_inflight` (the lockstep beam-search calls only);
    allowed_phrases: the strings of `--eval_allowed_phrases` (the lockstep beam search only; tokenised once, here); consensus /
    consensus_metric: `--eval_sample_consensus` / `--eval_consensus_metric` (the prediction is the consensus choice among that many
    samples instead of the beam search's); guidance_scale / guidance_alpha: `--eval_guidance_scale` / `--eval_guidance_alpha` (the
    lockstep calls only; the alpha reaches the sampling calls alone)"""
    _check_guidance(guidance_scale, guidance_alpha, batched or beam_groups > 1, eval_sample or best_of or consensus, sample_inflight or beam_inflight)
    if guidance_scale != 1.0 or guidance_alpha != 0.0:                       # flags absent: the calls below are unchanged
        beam_guide = {"guidance_scale": guidance_scale} if guidance_scale != 1.0 else {}
        sample_guide = dict(beam_guide, **({"guidance_alpha": guidance_alpha} if guidance_alpha else {}))
    else:
        beam_guide = sample_guide = {}
    module = getattr(model, "module", model)
    module.eval()
    trie = None
    if allowed_phrases:
        if not batched or beam_groups > 1 or best_of:
            raise ValueError("--eval_allowed_phrases needs --eval_batched_beam, without --eval_beam_groups and --eval_sample_best_of")
        from youku_mplug_amd import generation
        from youku_mplug_amd.downstream import _encode_phrase
        trie = generation.as_phrase_trie(list(allowed_phrases), generation._gen_config(module.text_decoder).vocab_size,
                                         lambda s: _encode_phrase(tokenizer, s))
    kvkw = {"kv_cache": "shared_prefix"} if shared_kv else {}                # flag absent: the calls below are unchanged
    kvkw.update(constraints or {})
    if mixed_prompts and not (batched or beam_groups > 1):
        raise ValueError("--eval_mixed_prompts needs --eval_batched_beam or --eval_beam_groups: the per-clip search has one prompt per call")
    mixkw = dict({"mixed_prompts": True} if mixed_prompts else {}, **beam_guide)    # flags absent: the calls below are unchanged
    if consensus and (best_of or beam_groups > 1 or allowed_phrases):
        raise ValueError("--eval_sample_consensus, --eval_sample_best_of, --eval_beam_groups and --eval_allowed_phrases all choose the "
                         "prediction: pass one of them")
    if sample_mixed_prompts and not ((eval_sample or best_of or consensus) and shared_kv):
        raise ValueError("--eval_sample_mixed_prompts needs --eval_sample or --eval_sample_best_of, and --eval_shared_kv")
    smixkw = dict({"sample_mixed_prompts": True} if sample_mixed_prompts else {}, **sample_guide)   # flags absent: the calls below are unchanged
    if sample_inflight and (sample_mixed_prompts or not ((eval_sample or best_of or consensus) and shared_kv)):
        raise ValueError("--eval_sample_inflight needs --eval_sample or --eval_sample_best_of, and --eval_shared_kv, without "
                         "--eval_sample_mixed_prompts")
    if sample_inflight:
        smixkw = {"inflight": True}
    if beam_inflight:
        _check_beam_inflight(batched, shared_kv, mixed_prompts, eval_sample or best_of or consensus or sample_mixed_prompts or sample_inflight)
        mixkw = {"beam_inflight": True}
    result = []
    for n, (video, video_ids, gold_caption) in enumerate(data_loader):
        video = video.to(device, non_blocking=True).bfloat16()
        text = [config["prompt"] for _ in range(video.shape[0])]
        text_input = tokenizer(text, padding="max_length", truncation=True, max_length=20, return_tensors="pt").to(device)
        qkw = {"decode_weights": "fp8"} if fp8_decode else {}                    # flag absent: the calls below are unchanged
        if score_gold:
            qf = module.encode_video(video)
            qkw = dict(qkw, query_features=qf)
        candidates = None
        if beam_groups > 1:
            per_group = min(5, 16 // beam_groups)
            candidates, _ = module.generate(video, text_input, batched=True, clips_per_search=clips_per_search, beam_groups=beam_groups,
                                            diversity_penalty=diversity_penalty, beam_size=per_group, num_return_gen=beam_groups * per_group,
                                            rerank_by_logprob=True, **kvkw, **qkw, **mixkw)
            res = [c[:1] for c in candidates]
        elif best_of:
            res = module.generate(video, text_input, do_sample=True, num_samples=best_of, best_of=True, seed=seed + n,
                                  clips_per_search=clips_per_search, **kvkw, **qkw, **smixkw)
        elif consensus:
            res = module.generate(video, text_input, do_sample=True, num_samples=consensus, consensus=consensus_metric, seed=seed + n,
                                  clips_per_search=clips_per_search, **kvkw, **qkw, **smixkw)
        elif trie is not None:
            res, phrase_info = module.generate(video, text_input, batched=True, clips_per_search=clips_per_search, allowed_phrases=trie,
                                               num_return_gen=min(5, trie.n_phrases), **kvkw, **qkw, **mixkw)
        else:
            res = module.generate(video, text_input, batched=True, clips_per_search=clips_per_search, **kvkw, **qkw, **mixkw) if batched else module.generate(video, text_input, **qkw)
        def caption(ids):
            ans = tokenizer.decode(ids).replace(" ", "").strip()
            return ans.split(config["prompt"])[-1].strip() if config["prompt"] != "" else ans
        for video_id, r, gold in zip(video_ids, res, gold_caption):
            result.append({"video_id": video_id, "pred_caption": caption(r.tolist()[0]), "gold_caption": list(gold)})
        if trie is not None:
            for rec, info in zip(result[-len(res):], phrase_info):
                rec["pred_candidates"] = [{"caption": allowed_phrases[i], "phrase_index": i, "score": float(sc)}
                                          for i, sc in zip(info["phrase_index"].tolist(), info["scores"].tolist())]
                rec["pred_caption"] = rec["pred_candidates"][0]["caption"] if rec["pred_candidates"] else ""
        if candidates is not None:
            for rec, rows in zip(result[-len(candidates):], candidates):
                rec["pred_candidates"] = [caption(row) for row in rows.tolist()]
        if eval_sample:
            sampled = module.generate(video, text_input, do_sample=True, num_samples=eval_sample, seed=seed + n, clips_per_search=clips_per_search,
                                      **kvkw, **qkw, **smixkw)
            for rec, rows in zip(result[-len(sampled):], sampled):
                rec["sampled_captions"] = [caption(row) for row in rows.tolist()]
        if score_gold:
            scores = module.score_captions(None, text_input, [gold_tokens(tokenizer, config["prompt"], g, max_length) for g in gold_caption],
                                           query_features=qf, clips_per_pass=clips_per_search)
            for rec, sc in zip(result[-len(scores):], scores):
                rec["gold_logprob"] = [float(x) for x in sc["sum_logprob"].tolist()]
                rec["gold_tokens"] = [int(x) for x in sc["count"].tolist()]
        if n == 0:
            print(result)
    return result


def _check_guidance(scale, alpha, beams, sampling, inflight):
    if not (math.isfinite(scale) and scale >= 0.0) or not 0.0 <= alpha < 1.0:
        raise ValueError(f"--eval_guidance_scale must be finite and not negative, --eval_guidance_alpha in [0, 1) (got {scale}, {alpha})")
    if scale == 1.0 and alpha == 0.0:
        return
    if not (beams or sampling) or inflight:
        raise ValueError("--eval_guidance_scale / --eval_guidance_alpha need a lockstep call (--eval_batched_beam, --eval_beam_groups, "
                         "--eval_sample, --eval_sample_best_of, --eval_sample_consensus), without --eval_sample_inflight and --eval_beam_inflight")
    if alpha and not sampling:
        raise ValueError("--eval_guidance_alpha acts on the sampling calls only (--eval_sample, --eval_sample_best_of, --eval_sample_consensus)")


def _check_beam_inflight(batched, shared_kv, mixed_prompts, sampling):
    if not (batched and shared_kv) or mixed_prompts or sampling:
        raise ValueError("--eval_beam_inflight needs --eval_batched_beam and --eval_shared_kv, without --eval_mixed_prompts and without "
                         "the sampling flags (--eval_sample, --eval_sample_best_of, --eval_sample_mixed_prompts, --eval_sample_inflight)")


def gold_tokens(tokenizer, prompt, captions, max_length):
    """the caption tokens of a clip's gold captions as the training pairs hold them ([prompt, caption] -> bos + prompt + caption + eos,
    make_training_batch): what lies between the prompt and the closing eos"""
    if not len(captions):
        return []
    enc = tokenizer([[prompt, c] for c in captions], padding="max_length", truncation=True, max_length=max_length, return_tensors="pt")
    eos = tokenizer.tokenizer.eos
    out = []
    for row, mask, pl in zip(enc["input_ids"].tolist(), enc["attention_mask"].tolist(), enc["prompt_lengths"].tolist()):
        n = sum(mask)
        end = n - 1 if n > 0 and row[n - 1] == eos else n
        out.append(row[1 + int(pl):end])
    return out


def gold_perplexity(result):
    """corpus per-token NLL and perplexity of the gold captions of `--eval_score_gold` result entries (terminators included)"""
    lp = sum(x for r in result for x in r.get("gold_logprob", []))
    nt = sum(x for r in result for x in r.get("gold_tokens", []))
    nll = -lp / max(nt, 1)
    return {"gold_nll": nll, "gold_ppl": math.exp(min(nll, 700.0)), "gold_scored_tokens": nt}


def save_result(result, result_dir, filename):
    """per-rank JSON, then rank 0 concatenates them in rank order (dataset/utils.py:114-160) -> path of the merged file"""
    rank, world = dist.get_rank(), dist.get_world_size()
    json.dump(result, open(os.path.join(result_dir, "%s_rank%d.json" % (filename, rank)), "w"))
    final = os.path.join(result_dir, "%s.json" % filename)
    dist.barrier()
    if rank == 0:
        merged = []
        for r in range(world):
            merged += json.load(open(os.path.join(result_dir, "%s_rank%d.json" % (filename, r)), "r"))
        json.dump(merged, open(final, "w"))
        print("result file saved to %s" % final)
    dist.barrier()
    return final


def normalize(text):
    """keep the CJK characters, one token each (:240-244)"""
    return " ".join(re.sub("[^\u4e00-\u9fa5]+", "", text))


def _ngrams(tokens, n):
    return Counter(tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1))


def bleu_scores(pairs, max_n=4):
    """Corpus BLEU-1..max_n as pycocoevalcap's Bleu scorer computes it (option 'closest'): clipped n-gram counts against the
    references' maximum counts summed over the corpus, brevity penalty from the summed closest reference lengths; the 1e-9 / 1e-15
    guards keep an empty numerator from producing log(0), as there."""
    tiny, small = 1e-15, 1e-9
    guess, correct = [0] * max_n, [0] * max_n
    test_len = ref_len = 0
    for hyp, refs in pairs:
        test_len += len(hyp)
        ref_len += min((abs(len(r) - len(hyp)), len(r)) for r in refs)[1]
        for n in range(1, max_n + 1):
            h = _ngrams(hyp, n)
            best = Counter()
            for r in refs:
                for g, c in _ngrams(r, n).items():
                    best[g] = max(best[g], c)
            guess[n - 1] += max(0, len(hyp) - n + 1)
            correct[n - 1] += sum(min(c, best[g]) for g, c in h.items())
    bp = 1.0 if test_len >= ref_len else math.exp(1 - ref_len / (test_len + small))
    out, logsum = [], 0.0
    for n in range(max_n):
        logsum += math.log((correct[n] + tiny) / (guess[n] + small))
        out.append(bp * math.exp(logsum / (n + 1)))
    return out


def rouge_l(pairs, beta=1.2):
    """mean over clips of the F-measure of the longest common subsequence, precision and recall each maximised over the references
    (pycocoevalcap's Rouge)"""
    def lcs(a, b):
        row = [0] * (len(b) + 1)
        for x in a:
            prev = 0
            for j, y in enumerate(b, 1):
                prev, row[j] = row[j], (prev + 1 if x == y else max(row[j], row[j - 1]))
        return row[-1]
    scores = []
    for hyp, refs in pairs:
        p = max((lcs(hyp, r) / len(hyp) if hyp else 0.0) for r in refs)
        rc = max((lcs(hyp, r) / len(r) if r else 0.0) for r in refs)
        scores.append((1 + beta ** 2) * p * rc / (rc + beta ** 2 * p) if p > 0 and rc > 0 else 0.0)
    return sum(scores) / max(len(scores), 1)


def corpus_cider(pairs, device):
    """Corpus CIDEr of [(hypothesis units, [reference units, ...])] -- one hypothesis per clip, units any hashable tokens (CJK
    characters here) -- as the reference project's scorer computes it: the units become ids in order of first appearance, the
    document frequencies come from THESE references, one ops.caption_cider call scores every clip, -> the mean over clips.
    ValueError: more than 65 535 distinct units, a caption of more than 255 units, a clip without references, no clip at all."""
    from youku_mplug_amd import generation, ops
    ids = {}
    enc = lambda cap: [ids.setdefault(u, len(ids)) for u in cap]
    hyps, refs = [enc(h) for h, _ in pairs], [[enc(r) for r in rs] for _, rs in pairs]
    if not pairs or any(not rs for rs in refs):
        raise ValueError("corpus CIDEr needs at least one clip, and references for every clip")
    if len(ids) > generation.CiderStats.MAX_VOCAB:
        raise ValueError(f"{len(ids)} distinct units do not fit the 16-bit key fields of the corpus table")
    stats = generation.CiderStats(refs, max(len(ids), 1))
    term = len(ids)                                                       # no unit has this id: it only pads
    flat = [r for rs in refs for r in rs]

    def table(caps):
        w = max(max(len(c) for c in caps), 1)
        return torch.tensor([c + [term] * (w - len(c)) for c in caps], dtype=torch.int64).to(device)
    begin_b = [0]
    for rs in refs:
        begin_b.append(begin_b[-1] + len(rs))
    _, score = ops.caption_cider(table(hyps), [0] * len(hyps), list(range(len(hyps) + 1)), table(flat), [0] * len(flat), begin_b,
                                 term=term, stats=stats)
    return float(score.mean().item())


def cal_metric(result_file, device=None):
    """(:246-298) first prediction per video id; predictions and references normalised to CJK characters"""
    result_list = json.load(open(result_file, "r"))
    seen, preds, golds = set(), {}, {}
    for each in result_list:
        if each["video_id"] in seen:
            continue
        seen.add(each["video_id"])
        preds[each["video_id"]] = normalize(each["pred_caption"])
        golds[each["video_id"]] = [normalize(c) for c in each["gold_caption"]]
    try:
        from pycocoevalcap.eval import COCOEvalCap
        from pycocotools.coco import COCO
    except ImportError:
        pairs = [(preds[k].split(), [g.split() for g in golds[k]]) for k in preds]
        b = bleu_scores(pairs)
        stats = {"Bleu_1": b[0], "Bleu_2": b[1], "Bleu_3": b[2], "Bleu_4": b[3], "ROUGE_L": rouge_l(pairs)}
        why = "a CPU run" if device is None or torch.device(device).type != "cuda" else None
        if why is None:
            try:
                stats["CIDEr"] = corpus_cider(pairs, device)
            except ValueError as e:
                why = str(e)
        if why is None:
            return {**stats, "scorer": "built-in BLEU / ROUGE-L, CIDEr on the device (pycocoevalcap not installed: no METEOR)"}
        return {**stats, "scorer": f"built-in BLEU / ROUGE-L (pycocoevalcap not installed: no METEOR / CIDEr; no device CIDEr: {why})"}
    stem = os.path.basename(result_file).replace(".json", "")
    pred_file, gt_file = "/tmp/%s_coco_format.json" % stem, "/tmp/%s_gt_file.json" % stem
    json.dump([{"image_id": k, "caption": v} for k, v in preds.items()], open(pred_file, "w"), ensure_ascii=False)
    gt = {"annotations": [], "images": [{"id": k, "file_name": k} for k in golds], "type": None, "info": None, "licenses": None}
    for k, caps in golds.items():
        for cap in caps:
            gt["annotations"].append({"image_id": k, "caption": cap, "id": len(gt["annotations"])})
    json.dump(gt, open(gt_file, "w"), ensure_ascii=False)
    coco = COCO(gt_file)
    coco_res = coco.loadRes(pred_file)
    ev = COCOEvalCap(coco, coco_res)
    ev.params["image_id"] = coco_res.getImgIds()
    ev.evaluate()
    return ev.eval


def synthetic_loaders(args, config, seed):
    """(clip, caption) training batches; (clip, video ids, [gold captions]) evaluation batches (test_collect_fn, :46-52)"""
    bs, frames, res = config["batch_size"], config["num_frames"], config["image_res"]

    def split(n, s, train):
        caps = ft.synthetic_titles(2 * n, max(4, config["max_length"] // 4), torch.Generator().manual_seed(s))
        if train:
            return ft.SyntheticSplit(n, bs, frames, res, s, lambda i: (caps[i],), drop_last=True)
        return ft.SyntheticSplit(n, bs, frames, res, s, lambda i: (f"video{s}_{i}", [caps[i], caps[n + i]]), collate=list)
    return split(args.synthetic_steps * args.update_freq * bs, seed, True), split(bs + 1, 1001, False), split(bs // 2 + 1, 1002, False)


def real_loaders(args, config):
    from dataset import create_dataset, create_loader, create_sampler
    from models.modeling_distributed_gpt3 import DistributedGPT3Tokenizer

    def test_collect_fn(batch):
        videos, ids, golds = zip(*batch)
        return torch.stack(videos, dim=0), list(ids), list(golds)
    datasets = create_dataset("video_caption", config)
    samplers = create_sampler(datasets, [True, False, False], dist.get_world_size(), dist.get_rank())
    loaders = create_loader(datasets, samplers, batch_size=[args.batch_size] * 3, num_workers=[args.num_workers] * 3,
                            is_trains=[True, False, False], collate_fns=[None, test_collect_fn, test_collect_fn])
    return loaders, DistributedGPT3Tokenizer(config["text_decoder"])


def main(args, config):
    s = ft.setup(args, config, lambda: real_loaders(args, config))
    if s.loaders is None:
        s.loaders = synthetic_loaders(args, config, s.seed)
    ft.build_engine(args, config, DistributedGPT3_Caption, s)
    data_loader, val_loader, _test_loader = s.loaders

    def step_fn(batch):
        video, text = batch
        return {"loss_generation": s.model(*make_training_batch(video, text, config["prompt"], s.tokenizer, s.device, args.max_length))}

    if getattr(args, "scst", False) and not args.evaluate_only:
        step_fn = scst_step_fn(args, config, s, data_loader)

    def evaluate_merged(*a, **kw):                                # generation and score_captions leave forward_lm: adapters, if any, are merged
        with ft.lora_merged_for_eval(s.model):
            return evaluation(*a, **kw)

    if args.evaluate_only:
        result = evaluate_merged(s.model, val_loader, s.tokenizer, s.device, config, batched=getattr(args, "eval_batched_beam", False),
                            clips_per_search=getattr(args, "clips_per_search", 32), eval_sample=getattr(args, "eval_sample", 0),
                            seed=getattr(args, "seed", 0) or 0, shared_kv=getattr(args, "eval_shared_kv", False),
                            constraints=constraint_keywords(args), best_of=getattr(args, "eval_sample_best_of", 0),
                            **({"beam_groups": args.eval_beam_groups, "diversity_penalty": args.eval_diversity_penalty}
                               if getattr(args, "eval_beam_groups", 1) > 1 else {}),
                            **({"score_gold": True, "max_length": args.max_length} if getattr(args, "eval_score_gold", False) else {}),
                            **({"fp8_decode": True} if getattr(args, "eval_fp8_decode", False) else {}),
                            **({"mixed_prompts": True} if getattr(args, "eval_mixed_prompts", False) else {}),
                            **({"sample_mixed_prompts": True} if getattr(args, "eval_sample_mixed_prompts", False) else {}),
                            **({"sample_inflight": True} if getattr(args, "eval_sample_inflight", False) else {}),
                            **({"beam_inflight": True} if getattr(args, "eval_beam_inflight", False) else {}),
                            **({"consensus": args.eval_sample_consensus, "consensus_metric": args.eval_consensus_metric or "rouge_l"}
                               if getattr(args, "eval_sample_consensus", 0) else {}),
                            **({"guidance_scale": args.eval_guidance_scale, "guidance_alpha": args.eval_guidance_alpha}
                               if getattr(args, "eval_guidance_scale", 1.0) != 1.0 or getattr(args, "eval_guidance_alpha", 0.0) != 0.0 else {}),
                            **({"allowed_phrases": read_phrases(args.eval_allowed_phrases)} if getattr(args, "eval_allowed_phrases", None) else {}))
        final = save_result(result, args.result_dir, "val_caption_result")
        val_stats = cal_metric(final, s.device)
        if getattr(args, "eval_score_gold", False):
            val_stats = {**val_stats, **gold_perplexity(json.load(open(final, "r")))}        # the merged file: every rank's clips
        print("* Validation Stats:", val_stats)
        log_stats = {**{f"val_{k}": v for k, v in val_stats.items()}, "n_parameters": s.n_parameters}
        ft.write_log(args, log_stats)
        return log_stats
    return ft.epoch_loop(args, s, step_fn, lambda epoch: {})


def training_captions(data_loader):
    """the training set's captions, one list per clip, without touching a video: the synthetic split's fields, or the `ann` list of
    the reference's caption datasets (a string or a list of strings under "caption")"""
    ds = data_loader.dataset
    if hasattr(ds, "fields"):
        return [[ds.fields(i)[0]] for i in range(ds.n)]
    if hasattr(ds, "ann"):
        return [list(a["caption"]) if isinstance(a["caption"], (list, tuple)) else [a["caption"]] for a in ds.ann]
    raise ValueError("--scst: the training set exposes no captions (no `ann` list): pass --scst_stats FILE, a saved generation.CiderStats")


def scst_step_fn(args, config, s, data_loader):
    """`--scst`: the training step as self-critical sequence training.  The rewards' corpus statistics are loaded (--scst_stats) or
    built here, once, from the training set's captions as the training pairs tokenise them (gold_tokens); a step is ONE forward_scst
    call over the batch -- prompts of different lengths in a batch are refused there -- and a clip's reference is its own caption."""
    from types import SimpleNamespace

    from youku_mplug_amd import generation
    module = getattr(s.model, "module", s.model)
    vocab = generation._gen_config(module.text_decoder).vocab_size
    prompt = config["prompt"]
    if getattr(args, "scst_stats", None):
        stats = generation.CiderStats.load(args.scst_stats)
    else:
        stats = generation.CiderStats([gold_tokens(s.tokenizer, prompt, caps, args.max_length) for caps in training_captions(data_loader)], vocab)
    print(f"SCST: CIDEr statistics over {stats.clips} clips, {stats.entries} n-grams in {stats.capacity} slots")
    kw = dict(cider=stats, num_samples=getattr(args, "scst_samples", 5), baseline=getattr(args, "scst_baseline", "mean_others"),
              temperature=getattr(args, "scst_temperature", 1.0))
    if getattr(args, "scst_shared_prefix", False):
        kw["training_pass"] = "shared_prefix"

    steps = [0]

    def step_fn(batch):
        video, text = batch
        video, text_input = make_training_batch(video, text, prompt, s.tokenizer, s.device, args.max_length)
        refs = [gold_tokens(s.tokenizer, prompt, [c], args.max_length) for c in text]
        # the prompt of a rollout: bos + the prompt's tokens, what generate's prompt of mask.sum() - 1 tokens is at evaluation.  The
        # tokenizer shortens the prompt of an over-long pair: a batch whose prompts then differ in length is refused by forward_scst
        # (one backward per step: the backward kernels overwrite .grad, so a step cannot be the sum of several forward_scst calls)
        col = torch.arange(text_input["input_ids"].shape[1], device=s.device)[None]
        mask = (col <= text_input["prompt_lengths"].to(s.device)[:, None] + 1).to(text_input["attention_mask"].dtype)
        loss, st = module.forward_scst(video, SimpleNamespace(input_ids=text_input["input_ids"], attention_mask=mask), refs, **kw)
        if dist.get_rank() == 0 and steps[0] % 10 == 0:                  # the loop's own print frequency
            print(f"SCST step {steps[0]}: reward {st['reward']:.4f} baseline {st['baseline']:.4f} length {st['length']:.2f} "
                  f"terminated {st['terminated']:.2f}")
        steps[0] += 1
        return {"loss_scst": loss}
    return step_fn


def read_phrases(path):
    """the phrases of an --eval_allowed_phrases file: one per line, surrounding blanks and blank lines dropped"""
    phrases = [line.strip() for line in open(path, "r", encoding="utf-8")]
    phrases = [p for p in phrases if p]
    if not phrases:
        raise ValueError(f"--eval_allowed_phrases: {path} holds no phrase")
    return phrases


def constraint_keywords(args):
    """the model.generate keywords of --eval_repetition_penalty / --eval_no_repeat_ngram / --eval_min_new_tokens; {} when all are off"""
    kw = {}
    if getattr(args, "eval_repetition_penalty", None) is not None:
        kw["repetition_penalty"] = args.eval_repetition_penalty
    if getattr(args, "eval_no_repeat_ngram", 0):
        kw["no_repeat_ngram_size"] = args.eval_no_repeat_ngram
    if getattr(args, "eval_min_new_tokens", 0):
        kw["min_new_tokens"] = args.eval_min_new_tokens
    if kw and not (getattr(args, "eval_batched_beam", False) or getattr(args, "eval_sample", 0) or getattr(args, "eval_sample_best_of", 0) or
                   getattr(args, "eval_sample_consensus", 0) or getattr(args, "eval_beam_groups", 1) > 1):
        raise ValueError(f"--eval_repetition_penalty / --eval_no_repeat_ngram / --eval_min_new_tokens ({kw}) need --eval_batched_beam or "
                         "--eval_sample (or --eval_sample_best_of): the per-clip beam search has no constraints")
    return kw


def get_args(argv=None):
    def extra(p):
        p.add_argument("--no_zero_shot", action="store_true")
        p.add_argument("--eval_batched_beam", action="store_true", default=False,
                       help="evaluation: beam-search the clips of a batch in lockstep (model.generate(batched=True)) instead of one by one")
        p.add_argument("--clips_per_search", type=int, default=32,
                       help="--eval_batched_beam: clips per lockstep search (KV memory: clips x beams x 2 cache copies)")
        p.add_argument("--eval_sample", type=int, default=0,
                       help="evaluation: also write N sampled captions per clip (model.generate(do_sample=True, num_samples=N))")
        p.add_argument("--eval_shared_kv", action="store_true", default=False,
                       help="--eval_batched_beam / --eval_sample: cache the query slots and the prompt once per clip "
                            "(model.generate(kv_cache='shared_prefix')) instead of once per beam or sample")
        p.add_argument("--eval_repetition_penalty", type=float, default=None,
                       help="--eval_batched_beam / --eval_sample: CTRL repetition penalty on the tokens generated so far (model.generate(repetition_penalty=F))")
        p.add_argument("--eval_no_repeat_ngram", type=int, default=0,
                       help="--eval_batched_beam / --eval_sample: no n-gram of N tokens is generated twice (model.generate(no_repeat_ngram_size=N))")
        p.add_argument("--eval_min_new_tokens", type=int, default=0,
                       help="--eval_batched_beam / --eval_sample: no termination token before N generated tokens (model.generate(min_new_tokens=N))")
        p.add_argument("--eval_sample_best_of", type=int, default=0,
                       help="evaluation: the caption of a clip is the most likely of N sampled ones, not the beam search's "
                            "(model.generate(do_sample=True, num_samples=N, best_of=True)); 0 = off")
        p.add_argument("--eval_sample_consensus", type=int, default=0,
                       help="evaluation: the caption of a clip is the consensus (minimum-Bayes-risk) choice among N sampled ones, the "
                            "sample that agrees most with the others, not the beam search's "
                            "(model.generate(do_sample=True, num_samples=N, consensus=METRIC)); 0 = off")
        p.add_argument("--eval_consensus_metric", type=str, default=None, choices=("rouge_l", "ngram_f"),
                       help="--eval_sample_consensus: the agreement, over token ids -- ROUGE-L (beta 1.2; the default) or the mean F of the "
                            "clipped 1..4-gram matches")
        p.add_argument("--eval_beam_groups", type=int, default=1,
                       help="evaluation: diverse beam search in lockstep, G groups of min(5, 16 // G) beams, the hypotheses re-ranked by the "
                            "model's log-probability per token (model.generate(batched=True, beam_groups=G, rerank_by_logprob=True)); 1 = off")
        p.add_argument("--eval_diversity_penalty", type=float, default=0.0,
                       help="--eval_beam_groups: what a later group pays for a token an earlier group chose at the same step "
                            "(model.generate(diversity_penalty=F))")
        p.add_argument("--eval_fp8_decode", action="store_true", default=False,
                       help="evaluation: the decode steps of every generation call run on e4m3 codes of the decoder's weights "
                            "(model.generate(decode_weights='fp8'))")
        p.add_argument("--eval_mixed_prompts", action="store_true", default=False,
                       help="--eval_batched_beam / --eval_beam_groups with --eval_shared_kv: one lockstep search per chunk of clips whatever "
                            "their prompt lengths (model.generate(mixed_prompts=True)) instead of one per distinct length")
        p.add_argument("--eval_sample_mixed_prompts", action="store_true", default=False,
                       help="--eval_sample / --eval_sample_best_of with --eval_shared_kv: one lockstep sampling loop per chunk of clips "
                            "whatever their prompt lengths (model.generate(do_sample=True, sample_mixed_prompts=True)) instead of one per "
                            "distinct length")
        p.add_argument("--eval_sample_inflight", action="store_true", default=False,
                       help="--eval_sample / --eval_sample_best_of with --eval_shared_kv: one sampling loop over all clips of a batch with "
                            "--clips_per_search clips resident, a finished clip's rows refilled with the next clip "
                            "(model.generate(do_sample=True, inflight=True))")
        p.add_argument("--eval_beam_inflight", action="store_true", default=False,
                       help="--eval_batched_beam with --eval_shared_kv: one beam search over all clips of a batch with --clips_per_search "
                            "clips resident, a finished clip's beams refilled with the next clip (model.generate(batched=True, beam_inflight=True))")
        p.add_argument("--eval_allowed_phrases", type=str, default=None, metavar="FILE",
                       help="--eval_batched_beam: the captions are phrases of FILE (one per line), found by a beam search along their trie "
                            "(model.generate(batched=True, allowed_phrases=...)); pred_candidates lists the best with their scores")
        p.add_argument("--eval_guidance_scale", type=float, default=1.0,
                       help="evaluation: the lockstep generation calls are guided by a null-video branch, cond + (F - 1) * (cond - uncond) "
                            "per step (model.generate(guidance_scale=F)); 1 = off")
        p.add_argument("--eval_guidance_alpha", type=float, default=0.0,
                       help="--eval_guidance_scale, sampling calls: ban the tokens whose probability is below F times the step's largest "
                            "(model.generate(guidance_alpha=F)); 0 = off")
        p.add_argument("--eval_score_gold", action="store_true", default=False,
                       help="evaluation: also score every clip's gold captions against its query features (model.score_captions): "
                            "gold_logprob / gold_tokens in the result file, per-token NLL and perplexity in the log")
        # self-critical training: absent from the namespace unless given (argparse.SUPPRESS), so a run without them is the run before them
        p.add_argument("--scst", action="store_true", default=argparse.SUPPRESS,
                       help="training: self-critical sequence training -- sample captions, reward them with CIDEr against the clip's own "
                            "caption on the device, weight their log-likelihood by reward minus baseline (model.forward_scst)")
        p.add_argument("--scst_samples", type=int, default=argparse.SUPPRESS, help="--scst: sampled captions per clip (default 5)")
        p.add_argument("--scst_baseline", type=str, default=argparse.SUPPRESS, choices=("mean_others", "greedy"),
                       help="--scst: the baseline of a sample's reward -- the mean reward of the clip's other samples (default), or the "
                            "reward of one greedy caption")
        p.add_argument("--scst_temperature", type=float, default=argparse.SUPPRESS, help="--scst: the sampling temperature (default 1.0)")
        p.add_argument("--scst_stats", type=str, default=argparse.SUPPRESS, metavar="FILE",
                       help="--scst: a saved generation.CiderStats (default: built at start-up from the training set's captions)")
        p.add_argument("--scst_shared_prefix", action="store_true", default=argparse.SUPPRESS,
                       help="--scst: the training pass computes every clip's query slots and prompt once and its samples as packed "
                            "continuations (forward_scst(training_pass='shared_prefix'); that pass applies no decoder dropout)")
    args, config = ft.get_args(argv, extra=extra)
    given = [k for k in ("scst_samples", "scst_baseline", "scst_temperature", "scst_stats", "scst_shared_prefix") if hasattr(args, k)]
    if given and not getattr(args, "scst", False):
        raise ValueError(f"--{' / --'.join(given)} need --scst")
    if getattr(args, "scst_samples", 5) < 1 or (getattr(args, "scst_samples", 5) < 2 and getattr(args, "scst_baseline", "mean_others") == "mean_others"):
        raise ValueError(f"--scst_samples must be at least 2 with --scst_baseline mean_others, at least 1 with greedy (got {args.scst_samples})")
    if not (math.isfinite(getattr(args, "scst_temperature", 1.0)) and getattr(args, "scst_temperature", 1.0) > 0):
        raise ValueError(f"--scst_temperature must be finite and positive (got {args.scst_temperature})")
    if args.eval_sample_best_of < 0:
        raise ValueError(f"--eval_sample_best_of must not be negative (got {args.eval_sample_best_of})")
    if args.eval_sample_consensus < 0:
        raise ValueError(f"--eval_sample_consensus must not be negative (got {args.eval_sample_consensus})")
    if args.eval_consensus_metric is not None and not args.eval_sample_consensus:
        raise ValueError("--eval_consensus_metric needs --eval_sample_consensus N")
    if args.eval_sample_consensus and (args.eval_sample_best_of or args.eval_beam_groups > 1 or args.eval_allowed_phrases):
        raise ValueError("--eval_sample_consensus, --eval_sample_best_of, --eval_beam_groups and --eval_allowed_phrases all choose the "
                         "prediction: pass one of them")
    if not 1 <= args.eval_beam_groups <= 8:
        raise ValueError(f"--eval_beam_groups must be in [1, 8] (got {args.eval_beam_groups})")
    if not (math.isfinite(args.eval_diversity_penalty) and args.eval_diversity_penalty >= 0) or \
            (args.eval_diversity_penalty and args.eval_beam_groups == 1):
        raise ValueError(f"--eval_diversity_penalty must be finite, not negative and needs --eval_beam_groups above 1 (got {args.eval_diversity_penalty})")
    if args.eval_beam_groups > 1 and args.eval_sample_best_of:
        raise ValueError("--eval_beam_groups and --eval_sample_best_of both choose the prediction: pass one of them")
    if args.eval_sample_mixed_prompts and not ((args.eval_sample or args.eval_sample_best_of or args.eval_sample_consensus) and args.eval_shared_kv):
        raise ValueError("--eval_sample_mixed_prompts needs --eval_sample N or --eval_sample_best_of N, and --eval_shared_kv")
    if args.eval_sample_inflight and (args.eval_sample_mixed_prompts or
                                      not ((args.eval_sample or args.eval_sample_best_of or args.eval_sample_consensus) and args.eval_shared_kv)):
        raise ValueError("--eval_sample_inflight needs --eval_sample N or --eval_sample_best_of N, and --eval_shared_kv, without "
                         "--eval_sample_mixed_prompts")
    _check_guidance(args.eval_guidance_scale, args.eval_guidance_alpha, args.eval_batched_beam or args.eval_beam_groups > 1,
                    args.eval_sample or args.eval_sample_best_of or args.eval_sample_consensus, args.eval_sample_inflight or args.eval_beam_inflight)
    if args.eval_beam_inflight:
        _check_beam_inflight(args.eval_batched_beam, args.eval_shared_kv, args.eval_mixed_prompts,
                             args.eval_sample or args.eval_sample_best_of or args.eval_sample_consensus or args.eval_sample_mixed_prompts or
                             args.eval_sample_inflight)
    if args.eval_allowed_phrases and (not args.eval_batched_beam or args.eval_beam_groups > 1 or args.eval_sample_best_of or
                                      args.eval_min_new_tokens):
        raise ValueError("--eval_allowed_phrases needs --eval_batched_beam, without --eval_beam_groups, --eval_sample_best_of and "
                         "--eval_min_new_tokens")
    constraint_keywords(args)                                               # refuses the flags without a lockstep mode
    config.setdefault("prompt", "")
    args.result_dir = os.path.join(args.output_dir, "result")
    os.makedirs(args.result_dir, exist_ok=True)
    return args, config


if __name__ == "__main__":
    main(*get_args())
