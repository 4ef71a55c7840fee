"""`--eval_on_device` and the model's search conveniences on the GPU: synthetic_retrieval_model at tiny dims, the on-device ranks
against itm_eval on the existing path's score matrices, single- and multi-target splits."""
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry():
    sys.path.insert(0, os.path.join(ROOT, "downstream"))
    sys.path.insert(0, ROOT)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(25000 + os.getpid() % 2000))
    import run_retrieval_distributed_gpt3 as entry
    return entry


def _model(dev, embed_dim=64):
    from oracle.weights import CONFIG_TINY, make_state_dict, retrieval_spec
    from youku_mplug_amd.retrieval import synthetic_retrieval_model
    model = synthetic_retrieval_model(CONFIG_TINY, device=dev)
    sd = make_state_dict(CONFIG_TINY, 2, spec_fn=retrieval_spec)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    return model.eval(), CONFIG_TINY


class _MultiSplit:
    """V clips, T > V titles; title t belongs to clip t % V, so a clip has 2-3 titles (the img2txt lists of the real datasets)"""

    def __init__(self, entry, cfg, V, T, bs, seed):
        base = entry.SyntheticRetrievalSet(T, bs, cfg.num_frames, cfg.img_size, 12, cfg.vocab, seed, False)
        self.text, self.V, self.bs, self.shape, self.seed = base.text, V, bs, base.shape, seed
        self.txt2vid = {t: t % V for t in range(T)}
        self.vid2txt = {v: [t for t in range(T) if t % V == v] for v in range(V)}
        self.dataset = self

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed + 1)
        for lo in range(0, self.V, self.bs):
            ids = list(range(lo, min(self.V, lo + self.bs)))
            yield torch.randn((len(ids),) + self.shape, generator=g), torch.tensor(ids)


def _no_near_ties(scores, D):
    """the precondition of the comparison: in every row of the existing path's matrix neighbouring scores are further apart than
    twice the summation-order bound b = D * 2^-24 * sum |q_i g_i| (tests/test_sim_topk_gpu.py); rows are unit vectors, so
    sum |q_i g_i| <= 1 (Cauchy-Schwarz) and b <= D * 2^-24.  Then the order of every row is certain."""
    gaps = np.diff(np.sort(scores, axis=1), axis=1)
    return gaps.size == 0 or gaps.min() > 2 * D * 2.0 ** -24 * 1.01          # 1 % for the bf16 rounding of the norms


def _compare(entry, model, split, dev, cfg):
    tok = entry.SyntheticTokenizer()
    conf = {"max_length": 12}
    v2t, t2v = entry.evaluation(model, split, tok, dev, conf)
    want = entry.itm_eval(v2t, t2v, split.txt2vid, split.vid2txt)
    rv, rt = entry.evaluation_on_device(model, split, tok, dev, conf)
    return v2t, t2v, want, rv, rt


@pytest.mark.parametrize("multi", [False, True])
def test_eval_on_device_equals_itm_eval(dev, multi):
    entry = _entry()
    model, cfg = _model(dev)
    picked = None
    # The split is chosen by a property of the EXISTING path's matrices alone.  The tiny random ViT maps gaussian clips to nearly
    # parallel features (median neighbouring gap of a text's video scores 1e-4, against 5e-3 for a video's text scores), so
    # the splits are small: 5 clips / 5 titles, or 4 clips / 10 titles, and the first seed whose matrices qualify is used.
    for seed in range(2000, 2032):
        split = _MultiSplit(entry, cfg, 4, 10, 2, seed) if multi else \
            entry.SyntheticRetrievalSet(5, 2, cfg.num_frames, cfg.img_size, 12, cfg.vocab, seed, False)
        v2t, t2v, want, rv, rt = _compare(entry, model, split, dev, cfg)
        D = model.vision_proj.out_features
        if _no_near_ties(v2t, D) and _no_near_ties(t2v, D):
            picked = seed
            break
    print("split seed", picked)
    assert picked is not None, "no synthetic split without near-ties among 32 seeds"
    assert rv.dtype == np.int32 and rv.shape == (v2t.shape[0],) and rt.shape == (t2v.shape[0],)
    # the ranks themselves, not only the recall counts: itm_eval's argsort position of the wanted row(s)
    lists = [split.vid2txt[v] for v in range(v2t.shape[0])]
    assert rv.tolist() == [min(int(np.where(np.argsort(s)[::-1] == t)[0][0]) for t in ts) for s, ts in zip(v2t, lists)]
    assert rt.tolist() == [int(np.where(np.argsort(s)[::-1] == split.txt2vid[i])[0][0]) for i, s in enumerate(t2v)]
    assert entry.recall_from_ranks(rv, rt) == want


def test_search_videos_and_texts_return_the_argmax(dev):
    from oracle.weights import make_inputs
    from youku_mplug_amd.retrieval import RetrievalIndex
    model, cfg = _model(dev)
    video, ids, mask = make_inputs(cfg, 12, 10, seed=11, ragged=True)
    video = video.to(dev).to(torch.bfloat16)
    text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    vf = torch.cat([model.extract_vision_feature(video[i:i + 4]) for i in range(0, 12, 4)])
    tf = model.extract_text_feature(text)
    assert vf.dtype == torch.bfloat16 and tf.dtype == torch.bfloat16           # .float() of the existing path is exact
    vindex, tindex = RetrievalIndex(vf.shape[1], device=dev, capacity=4), RetrievalIndex(tf.shape[1], device=dev, capacity=4)
    for i in range(0, 12, 4):
        vindex.add(vf[i:i + 4])
        tindex.add(tf[i:i + 4])
    s = tf.float() @ vf.float().t()
    scores, idx = model.search_videos(text, vindex, 3)
    assert torch.equal(idx[:, 0], torch.sort(-s, dim=1, stable=True).indices[:, 0])
    assert torch.allclose(scores[:, 0], s.max(dim=1).values, atol=1e-5, rtol=0)
    scores, idx = model.search_texts(video[:5], tindex, 2)
    st = vf[:5].float() @ tf.float().t()
    assert torch.equal(idx[:, 0], torch.sort(-st, dim=1, stable=True).indices[:, 0])
    assert torch.allclose(scores[:, 0], st.max(dim=1).values, atol=1e-5, rtol=0)
