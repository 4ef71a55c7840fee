"""The embedding fronts and the glue kernels of csrc/elementwise.hip and csrc/glue.hip -- patch im2col, ViT token assembly, cls merge
(full-tensor, fix-up and in-place forms), row / segment copies, add, column sums, the GPT embedding front with its dropout mask, the
log-prob top-k of beam search, the fp32 gradient window, store_words, the composed temporal projection's finishing steps, caption
targets, the KV-cache row gather -- against the fp64 references of tests/ref_embed_glue.py, element by element, at the smallest shapes
that reach each path and edge (the tables of tests/embed_glue_cases.py say which).  Gates: embed_glue_cases.GATES, every one derived
(number formats, the worst-case bound of an fp32 sum, the project's gate of the same log-sum-exp chain); pytest -s prints every
comparison's worst residual; profiles/embed_glue_kernel_errors.md holds the table.  Everything called a move, bit for bit, exact or
untouched is compared on the raw bits.
Run on the MI355X box: pytest -m gpu tests/test_embed_glue_kernels_gpu.py"""
import pytest

import embed_glue_cases as K

pytestmark = pytest.mark.gpu


def _cases(entry):
    runs = K.TABLES[entry][1]
    return pytest.mark.parametrize("name,args,kw", runs, ids=[r[0] for r in runs])


def _run(entry, dev, args, kw):
    from youku_mplug_amd import ops
    K.TABLES[entry][0](ops, dev, *args, **kw)


@_cases("im2col_patches")
def test_im2col_patches_bits(dev, name, args, kw):
    """both kernels of mpv_im2col_patches against the index-built reference, raw bits (embed_glue_cases.run_im2col)"""
    _run("im2col_patches", dev, args, kw)


@_cases("vit_embed_assemble_fwd")
def test_vit_embed_assemble_fwd_vs_fp64(dev, name, args, kw):
    _run("vit_embed_assemble_fwd", dev, args, kw)


@_cases("vit_embed_assemble_bwd")
def test_vit_embed_assemble_bwd_vs_fp64(dev, name, args, kw):
    """dpatch bits, dpos / dcls / dtemporal around the row lanes and column stripes of their kernels (run_assemble_bwd)"""
    _run("vit_embed_assemble_bwd", dev, args, kw)


@_cases("vit_cls_merge")
def test_vit_cls_merge_family_vs_fp64(dev, name, args, kw):
    """mpv_vit_cls_merge_fwd / _bwd against fp64; mpv_vit_cls_fix_fwd and mpv_vit_cls_merge_bwd_inplace bit-identical to them (run_cls_merge)"""
    _run("vit_cls_merge", dev, args, kw)


@_cases("copy_rows")
def test_copy_rows_bits(dev, name, args, kw):
    _run("copy_rows", dev, args, kw)


@_cases("add")
def test_add_vs_fp64(dev, name, args, kw):
    _run("add", dev, args, kw)


@_cases("colsum")
def test_colsum_vs_fp64(dev, name, args, kw):
    _run("colsum", dev, args, kw)


@_cases("gpt_embed")
def test_gpt_embed_fwd_bwd_vs_fp64_and_keep_mask(dev, name, args, kw):
    """values against fp64, the dropped positions against ref_norm.keep_mask exactly, in mpv_gpt_embed_fwd, _bwd and _bwd_full (run_gpt_embed)"""
    _run("gpt_embed", dev, args, kw)


@_cases("gpt_embed_bwd_full_wrap")
def test_gpt_embed_bwd_full_grid_wraps(dev, name, args, kw):
    _run("gpt_embed_bwd_full_wrap", dev, args, kw)


@_cases("gpt_embed_rows_fwd")
def test_gpt_embed_rows_fwd_vs_fp64(dev, name, args, kw):
    _run("gpt_embed_rows_fwd", dev, args, kw)


@_cases("logprob_topk")
def test_logprob_topk_indices_exact_values_vs_fp64(dev, name, args, kw):
    """indices == the stable descending order of the bf16 logits in EVERY row (ties, banned slices, dead beams); values against fp64
    (run_logprob_topk)"""
    _run("logprob_topk", dev, args, kw)


@_cases("copy_segments")
def test_copy_segments_bits(dev, name, args, kw):
    _run("copy_segments", dev, args, kw)


@_cases("accum_f32")
def test_accum_f32_bits(dev, name, args, kw):
    _run("accum_f32", dev, args, kw)


@_cases("f32_to_bf16")
def test_f32_to_bf16_bits(dev, name, args, kw):
    _run("f32_to_bf16", dev, args, kw)


@_cases("store_words")
def test_store_words_bits(dev, name, args, kw):
    _run("store_words", dev, args, kw)


@_cases("vit_compose")
def test_vit_compose_finish_and_bias_vs_fp64(dev, name, args, kw):
    """mpv_vit_compose_bwd_finish (+ _batched, bit-identical) and mpv_vit_compose_bias_batched (run_compose)"""
    _run("vit_compose", dev, args, kw)


@_cases("caption_targets")
def test_caption_targets_vs_fp64(dev, name, args, kw):
    _run("caption_targets", dev, args, kw)


@_cases("gather_rows_ld")
def test_gather_rows_ld_bits(dev, name, args, kw):
    _run("gather_rows_ld", dev, args, kw)
