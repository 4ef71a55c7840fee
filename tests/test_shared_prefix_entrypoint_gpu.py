"""--eval_shared_prefix in the ITM and classification entry points (downstream/run_retrieval_distributed_gpt3_itm.py,
downstream/run_cls_distributed_gpt3.py): `--evaluate_only` on synthetic data with and without it.  Both runs print their metrics, and
their score matrices agree within the gate of tests/test_shared_prefix_gpu.py."""
import pytest
import torch

from test_entrypoint_gpu import _finetune_entry, _write_finetune_config
from test_shared_prefix_gpu import _agree

pytestmark = pytest.mark.gpu


def test_itm_entrypoint_evaluates_through_the_shared_prefix(tmp_path, dev, monkeypatch, capsys):
    entry = _finetune_entry("run_retrieval_distributed_gpt3_itm")
    cfg = _write_finetune_config(str(tmp_path), "itm", "use_cls: true")
    mats = []
    orig = entry.evaluation
    monkeypatch.setattr(entry, "evaluation", lambda *a, **k: mats.append(orig(*a, **k)) or mats[-1])
    res = []
    for i, extra in enumerate(([], ["--eval_shared_prefix", "--eval_text_bs", "3"])):
        args, config = entry.get_args(["--config", cfg, "--output_dir", str(tmp_path / f"out{i}"), "--bf16", "--enable_deepspeed",
                                       "--synthetic_steps", "1", "--seed", "5", "--evaluate_only"] + extra)
        assert args.eval_shared_prefix == bool(extra) and args.eval_text_bs == (3 if extra else 8)
        res.append(entry.main(args, config)["val"])
        assert "Validation Performance:" in capsys.readouterr().out
    (g0, _, c0, _), (g1, _, c1, _) = mats
    _agree(torch.as_tensor(g1), torch.as_tensor(g0), "generation")
    _agree(torch.as_tensor(c1), torch.as_tensor(c0), "cls")
    assert set(res[0]) == set(res[1]) and all(0.0 <= v <= 100.0 for r in res for v in r.values())


def test_cls_entrypoint_evaluates_through_the_shared_prefix(tmp_path, dev, monkeypatch, capsys):
    from youku_mplug_amd.downstream import _GenCls
    entry = _finetune_entry("run_cls_distributed_gpt3")
    cfg = _write_finetune_config(str(tmp_path), "cls", "use_cls: true\nnum_classes: 6", batch_size=20)
    seen = {"plain": [], "shared": []}
    orig_scores, orig_shared = _GenCls._scores, _GenCls.score_shared_prefix
    monkeypatch.setattr(_GenCls, "_scores", lambda self, *a, **k: seen["plain"].append(orig_scores(self, *a, **k)) or seen["plain"][-1])
    monkeypatch.setattr(_GenCls, "score_shared_prefix",
                        lambda self, *a, **k: seen["shared"].append(orig_shared(self, *a, **k)) or seen["shared"][-1])
    logs = []
    for i, extra in enumerate(([], ["--eval_shared_prefix"])):
        args, config = entry.get_args(["--config", cfg, "--output_dir", str(tmp_path / f"out{i}"), "--bf16", "--enable_deepspeed",
                                       "--synthetic_steps", "1", "--seed", "6", "--evaluate_only"] + extra)
        assert args.eval_shared_prefix == bool(extra)
        logs.append(entry.main(args, config))
        out = capsys.readouterr().out
        assert "Generation Top-1 Accuracy" in out and "Validation Performance:" in out
    assert len(seen["plain"]) == len(seen["shared"]) > 0
    for k, name in ((0, "generation"), (1, "cls")):
        _agree(torch.cat([s[k] for s in seen["shared"]]), torch.cat([s[k] for s in seen["plain"]]), name)
    assert logs[0]["epoch"] == logs[1]["epoch"] == -1 and set(logs[0]) == set(logs[1])
