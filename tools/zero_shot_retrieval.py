"""Zero-shot video-text retrieval with a PRE-TRAINED checkpoint's contrastive head (use_contrastive: vision_proj, text_proj, temp):
recall@1/5/10 of titles against clips and clips against titles under the query-max score the head was trained with (the score of a
title and a clip is the max over the clip's num_learnable_token query features).

    python tools/zero_shot_retrieval.py --config configs/<pretrain>.yaml --checkpoint <ckpt.pth>      # the YAML's retrieval split
    python tools/zero_shot_retrieval.py --synthetic 24                                                  # random tiny model / split

Both indexes (retrieval.MaxSimIndex: clips [n, Q, E], titles [n, E]) are built over the split in batches, every query is ranked
against the whole gallery on the device by ops.maxsim_rank -- no score matrix anywhere -- and the itm_eval dictionary of the
retrieval entry point is printed as one JSON line.  recall_from_ranks, the synthetic split and the tokenizer are that entry
point's own (downstream/run_retrieval_distributed_gpt3.py), which is not changed."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _repo_first():
    """this repository's entry points in FRONT of sys.path: the retrieval entry point imports run_pretrain_distributed_gpt3 by name,
    and a checkout of the reference project further up the path has a module of that name too"""
    for p in (os.path.join(ROOT, "downstream"), ROOT):
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)


_repo_first()


def _entry():
    _repo_first()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(26000 + os.getpid() % 2000))
    import run_retrieval_distributed_gpt3 as entry
    return entry


@torch.no_grad()
def build_indexes(model, split, tokenizer, device, max_length, index_fp8=False):
    """-> (video index [clips, Q, E], text index [titles, E]) over the split, features extracted batch by batch.  index_fp8: the video
    index keeps e4m3 codes (half the bytes); the title index stays bf16 -- clips are searched against it with grouped queries, the
    direction an fp8 index does not serve, and it is 1 / Q of the bytes anyway."""
    from youku_mplug_amd.retrieval import MaxSimIndex
    model.eval()
    texts = split.dataset.text
    text_index = video_index = None
    for i in range(0, len(texts), 32):
        text_input = tokenizer(texts[i:i + 32], padding="max_length", truncation=True, max_length=max_length, return_tensors="pt").to(device)
        feat = model.extract_text_feature(text_input)
        text_index = text_index or MaxSimIndex(feat.shape[1], 1, device=device)
        text_index.add(feat)
    for video, _vid in split:
        feat = model.extract_vision_feature(video.to(device).bfloat16())
        video_index = video_index or MaxSimIndex(feat.shape[2], feat.shape[1], device=device, storage="fp8" if index_fp8 else "bf16")
        video_index.add(feat)
    return video_index, text_index


@torch.no_grad()
def zero_shot_ranks(model, split, tokenizer, device, max_length, index_fp8=False):
    """-> (ranks_v2t int32 [clips], ranks_t2v int32 [titles]) as numpy arrays, from MaxSimIndex.rank (ops.maxsim_rank; with index_fp8
    the title -> clip direction runs ops.maxsim_rank_q8 on the codes, and the clips that query the titles are the index's own
    dequantised rows, 1024 clips at a time)"""
    entry = _entry()
    video_index, text_index = build_indexes(model, split, tokenizer, device, max_length, index_fp8)
    print(f"index bytes: video {video_index.nbytes} ({video_index.storage}), text {text_index.nbytes} ({text_index.storage})")
    ds = split.dataset
    nv, nt = len(video_index), len(text_index)
    if index_fp8:
        ranks_v2t = torch.cat([text_index.rank((video_index.codes[i:i + 1024].view(torch.float8_e4m3fn).float()
                                                * video_index.scales[i:i + 1024, :, None]).to(torch.bfloat16),
                                               entry._targets(ds.vid2txt, range(i, min(i + 1024, nv)), device)) for i in range(0, nv, 1024)])
    else:
        ranks_v2t = text_index.rank(video_index.features, entry._targets(ds.vid2txt, range(nv), device))   # clip -> title: q_group = Q
    ranks_t2v = video_index.rank(text_index.features[:, 0], entry._targets(ds.txt2vid, range(nt), device))   # title -> clip: g_group = Q
    return ranks_v2t.cpu().numpy(), ranks_t2v.cpu().numpy()


def synthetic_setup(n, batch_size, device, seed, shapes=None):
    """random-weight contrastive pre-train model at tiny shapes and the retrieval entry point's synthetic split of n pairs"""
    from youku_mplug_amd.pretrain import synthetic_model
    entry = _entry()
    if shapes is None:
        from oracle.weights import CONFIG_TINY as shapes
    torch.manual_seed(seed)
    model = synthetic_model(shapes, device=device, use_contrastive=True)
    split = entry.SyntheticRetrievalSet(n, batch_size, shapes.num_frames, shapes.img_size, 12, shapes.vocab, seed, False)
    return model, split, entry.SyntheticTokenizer(), 12


def real_setup(args, device):
    import yaml
    entry = _entry()
    from run_pretrain_distributed_gpt3 import _ConfigLoader
    from youku_mplug_amd.pretrain import DistributedGPT3_Pretrain
    config = yaml.load(open(args.config, "r"), Loader=_ConfigLoader)
    if not config.get("use_contrastive", False):
        raise SystemExit(f"{args.config}: use_contrastive is not set; this checkpoint has no contrastive head to evaluate")
    try:
        from dataset import create_dataset, create_loader
        from models.modeling_distributed_gpt3 import DistributedGPT3Tokenizer
    except ImportError as e:
        raise SystemExit(f"real-data runs need the reference's `dataset` package and tokenizer on PYTHONPATH ({e}); use --synthetic N")
    datasets = create_dataset("video_retrieval", config)
    loaders = create_loader(datasets, [None] * 3, batch_size=[args.batch_size] * 3, num_workers=[args.num_workers] * 3,
                            is_trains=[False] * 3, collate_fns=[None] * 3)
    tokenizer = DistributedGPT3Tokenizer(config["text_decoder"])
    model = DistributedGPT3_Pretrain(config=config, tokenizer=tokenizer, device=device)
    if args.checkpoint:
        entry.load_resume_state(model, args.checkpoint)
    return model, loaders[{"train": 0, "val": 1, "test": 2}[args.split]], tokenizer, max(64, config.get("max_length", 64))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", help="pre-train YAML (use_contrastive: true)")
    ap.add_argument("--checkpoint", help="pre-training checkpoint ('model' or 'module' key)")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N synthetic (clip, title) pairs and a random tiny model")
    ap.add_argument("--split", default="test", choices=("train", "val", "test"))
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--index_fp8", action="store_true",
                    help="keep the video index as e4m3 codes with one scale per row (half the bytes); the title index stays bf16.  The "
                         "search results are exactly those of a bf16 index of the dequantised rows; what the rounding does to recall on "
                         "trained features has not been measured")
    args = ap.parse_args(argv)
    if not args.synthetic and not args.config:
        ap.error("give --config (and --checkpoint), or --synthetic N")
    device = torch.device(args.device)
    if args.synthetic:
        model, split, tokenizer, max_length = synthetic_setup(args.synthetic, args.batch_size, device, args.seed)
    else:
        model, split, tokenizer, max_length = real_setup(args, device)
    result = _entry().recall_from_ranks(*zero_shot_ranks(model, split, tokenizer, device, max_length, args.index_fp8))
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
