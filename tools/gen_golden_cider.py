"""Records what the reference project's own CIDEr scorer (refTools/evaluation/cider/cider_scorer.py, class CiderScorer) computes on the
cases of tests/cider_cases.py -> tests/golden/cider_reference.json.  Only recorded inputs and scores are written; nothing of the
scorer is copied.  The scorer is Python 2 (xrange, dict.iteritems): its source text is loaded from the reference tree
(oracle.ref_loader.REF_ROOT) and those two names are adapted IN MEMORY before it is executed.

The scorer scores ONE hypothesis per document, and a document's references define the corpus (df, log of the document count).  A case
has several candidates per clip, so the scorer is run once per candidate index k: every clip of the corpus is one document whose
hypothesis is the clip's k-th candidate (an empty string where the clip has fewer) -- the corpus, and so df and log_ref_len, are the
same in every run.  A clip without references is no document: its candidates score 0.0 by definition and are recorded so.

    python tools/gen_golden_cider.py          (needs the reference tree; tests never run this)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def load_scorer():
    from oracle.ref_loader import REF_ROOT
    path = os.path.join(REF_ROOT, "refTools", "evaluation", "cider", "cider_scorer.py")
    text = open(path).read().replace("xrange", "range").replace(".iteritems()", ".items()")
    ns = {"__name__": "cider_scorer_py3"}
    exec(compile(text, path, "exec"), ns)
    return ns["CiderScorer"]


def words(caption):
    return " ".join(str(t) for t in caption)


def run(CiderScorer, hyps, reference_sets):
    """one hypothesis per document -> (mean, per-document scores) by the scorer's compute_score"""
    scorer = CiderScorer(n=4, sigma=6.0)
    for h, refs in zip(hyps, reference_sets):
        scorer += (words(h), [words(r) for r in refs])
    mean, scores = scorer.compute_score()
    return float(mean), [float(s) for s in scores]


def main():
    import cider_cases as cc
    CiderScorer = load_scorer()
    out = {"cases": {}, "sigma": 6.0, "n": 4}
    for case in cc.CASES:
        docs = [g for g, refs in enumerate(case["groups_b"]) if refs]
        corpus = [case["groups_b"][g] for g in docs]
        assert corpus == case["corpus"]
        score = [[0.0] * len(c) for c in case["groups_a"]]
        for k in range(max(len(c) for c in case["groups_a"])):
            hyps = [case["groups_a"][g][k] if k < len(case["groups_a"][g]) else [] for g in docs]
            _, per_doc = run(CiderScorer, hyps, corpus)
            for g, s in zip(docs, per_doc):
                if k < len(case["groups_a"][g]):
                    score[g][k] = s
        out["cases"][case["name"]] = dict(candidates=case["groups_a"], references=case["groups_b"], score=score)
    mean, per_doc = run(CiderScorer, cc.EVAL_HYPS, cc.EVAL_REFS)
    out["eval"] = dict(hypotheses=cc.EVAL_HYPS, references=cc.EVAL_REFS, mean=mean, score=per_doc)
    path = os.path.join(ROOT, "tests", "golden", "cider_reference.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
