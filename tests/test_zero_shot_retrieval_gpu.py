"""Zero-shot retrieval from the contrastive pre-train model on the GPU at CONFIG_TINY: extract_*_feature against the loss path's
operands bit for bit, search_videos / search_texts and both rank vectors against argsort of the matrices mpv_maxsim_fwd produces
for the same features, and tools/zero_shot_retrieval.py --synthetic against itm_eval on those matrices."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_contrastive_gpu import build_contrastive, capture_itc_tapes      # noqa: E402  (the recipe, not its tests)
from test_retrieval_search_gpu import _no_near_ties                         # noqa: E402


def _tool():
    spec = importlib.util.spec_from_file_location("zero_shot_retrieval", os.path.join(ROOT, "tools", "zero_shot_retrieval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _batch(cfg, dev, n, seed):
    from oracle.weights import make_inputs
    video, ids, mask = make_inputs(cfg, n, 10, seed=seed, ragged=True)
    return video.to(dev).to(torch.bfloat16), types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))


def _matrices(vf, tf):
    """(clips x titles, titles x clips) fp32 by mpv_maxsim_fwd, unscaled"""
    from youku_mplug_amd import ops
    N, Q, E = vf.shape
    T = tf.shape[0]
    v2t, _ = ops.maxsim_fwd(vf.reshape(N * Q, E).contiguous(), tf.contiguous(), N, Q, T, E)
    t2v, _ = ops.maxsim_fwd(vf.reshape(N * Q, E).contiguous(), tf.contiguous(), N, Q, T, E, trans=True)
    return v2t, t2v


def test_features_equal_the_loss_operands_bit_for_bit(dev):
    from oracle.weights import CONFIG_TINY as cfg
    model = build_contrastive(cfg, dev, 2).eval()
    tapes = capture_itc_tapes(model)
    video, text = _batch(cfg, dev, 8, 21)
    with torch.no_grad():
        model(video, text)
    c = tapes[-1]["itc"]
    vf, tf = model.extract_vision_feature(video), model.extract_text_feature(text)
    Q, E = model.num_learnable_token, model.vision_proj.out_features
    assert vf.shape == (8, Q, E) and tf.shape == (8, E) and vf.dtype == tf.dtype == torch.bfloat16
    assert torch.equal(vf.reshape(8 * Q, E).view(torch.int16), c["vf"].view(torch.int16))
    assert torch.equal(tf.view(torch.int16), c["tf"].view(torch.int16))
    n = torch.cat([vf.reshape(-1, E), tf]).float().norm(dim=1)
    assert torch.allclose(n, torch.ones_like(n), atol=1e-2)


def test_search_and_ranks_equal_argsort_of_the_maxsim_fwd_matrices(dev):
    from oracle.weights import CONFIG_TINY as cfg
    from youku_mplug_amd.retrieval import MaxSimIndex
    model = build_contrastive(cfg, dev, 2).eval()
    E = model.vision_proj.out_features
    picked = None
    # The batch is chosen by a property of the EXISTING kernel's matrices alone.  The tiny random ViT maps gaussian clips to nearly
    # parallel features (tests/test_retrieval_search_gpu.py), so the galleries are small: the first N = 4 clips / titles of a batch
    # of 8 (the towers run at the batch size the loss runs at), queries are rows 0 .. 3 of the batch.
    N = 4
    for seed in range(3000, 3032):
        video, text = _batch(cfg, dev, 8, seed)
        vf, tf = model.extract_vision_feature(video), model.extract_text_feature(text)
        v2t, t2v = _matrices(vf[:N].contiguous(), tf[:N].contiguous())
        if _no_near_ties(v2t.cpu().numpy(), E) and _no_near_ties(t2v.cpu().numpy(), E):
            picked = seed
            break
    print("batch seed", picked)
    assert picked is not None, "no batch without near-ties among 32 seeds"
    vindex, tindex = MaxSimIndex(E, vf.shape[1], device=dev, capacity=2), MaxSimIndex(E, 1, device=dev, capacity=2)
    for i in range(0, N, 3):
        vindex.add(vf[i:min(N, i + 3)])
        tindex.add(tf[i:min(N, i + 3)])
    inv_temp = 1.0 / float(model.temp)
    s, i = model.search_videos(text, vindex, 3)
    order = torch.sort(-t2v, dim=1, stable=True).indices
    assert torch.equal(i[:N], order[:, :3])
    assert torch.allclose(s[:N], torch.gather(t2v, 1, order[:, :3]) * inv_temp, rtol=1e-6, atol=E * 2.0 ** -24 * inv_temp)
    s, i = model.search_texts(video, tindex, N)
    order = torch.sort(-v2t, dim=1, stable=True).indices
    assert torch.equal(i[:N], order)
    assert torch.allclose(s[:N], torch.gather(v2t, 1, order) * inv_temp, rtol=1e-6, atol=E * 2.0 ** -24 * inv_temp)
    want = lambda m: [int(np.where(np.argsort(r)[::-1] == j)[0][0]) for j, r in enumerate(m.cpu().numpy())]
    assert tindex.rank(vf[:N], torch.arange(N)).tolist() == want(v2t)
    assert vindex.rank(tf[:N], torch.arange(N)).tolist() == want(t2v)


def test_tool_synthetic_recalls_equal_itm_eval(dev, capsys):
    tool = _tool()
    entry = tool._entry()
    picked = None
    for seed in range(5000, 5032):
        model, split, tok, max_length = tool.synthetic_setup(6, 4, dev, seed)
        vi, ti = tool.build_indexes(model, split, tok, dev, max_length)
        v2t, t2v = _matrices(vi.features, ti.features[:, 0])
        E = vi.dim
        if _no_near_ties(v2t.cpu().numpy(), E) and _no_near_ties(t2v.cpu().numpy(), E):
            picked = seed
            break
    print("tool seed", picked)
    assert picked is not None, "no synthetic split without near-ties among 32 seeds"
    want = entry.itm_eval(v2t.cpu().numpy(), t2v.cpu().numpy(), split.txt2vid, split.vid2txt)
    capsys.readouterr()
    result = tool.main(["--synthetic", "6", "--batch_size", "4", "--seed", str(picked), "--device", str(dev)])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    assert json.loads(line) == result == want
