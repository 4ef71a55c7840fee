"""Guided caption decoding, checked without a GPU: the fp32 stand-in tests/standin_guidance.py against the fp64
reference tests/ref_guidance.py on every case of tests/guidance_cases.py, within a bound made of the three fp32 roundings and the final
bf16 one; the library's refusals on the host and the ctypes mirror of the descriptor; the kernel's resources; generation.GuidedState on
a recording state (the doubled prefill, the doubled tokens, the mirrored re-order, prompt_len exactly when the inner state takes it)
and on the stand-in states of the tiny model; every refusal; and "off means off": scale 1 with alpha 0 is the unguided call."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import guidance_cases as gc
import ref_guidance
import standin_guidance as stg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def _gen():
    from youku_mplug_amd import generation
    return generation


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------ the stand-in against the reference
@pytest.mark.parametrize("case", gc.KERNEL_CASES, ids=gc.case_id)
def test_standin_is_within_the_rounding_bound_of_the_fp64_reference(case):
    b = gc.build(case)
    V, scale, alpha = case["V"], case["scale"], case["alpha"]
    cond0, uncond0 = b["cond"].clone(), b["uncond"].clone()
    ref = ref_guidance.guide(cond0, uncond0, scale=scale, alpha=alpha, vocab=V)
    bound = ref_guidance.bound(ref, scale)
    # The ban compares c alone, which the rounding to bf16 at the end never touches: what may move an element across the threshold is
    # the fp32 part of the bound.  The case is one where no element is that close to it -- checked with the reference alone -- so the
    # ban sets must be equal.
    if alpha > 0.0:
        close = (ref["c"] - ref["plaus_log"]).abs() <= ref_guidance.fp32_slack(ref, scale)
        assert not bool(close.any()), "a centred logit of this case sits on the plausibility threshold"
    got = stg.logits_guide(b["cond"], b["uncond"], scale=scale, alpha=alpha, ban_value=case["ban"], vocab=V)
    assert got is b["cond"]
    assert torch.equal(_bits(b["uncond"]), _bits(uncond0)) and (got[:, V:] == gc.POISON).all() and torch.equal(_bits(got[:, V:]), _bits(cond0[:, V:]))
    out = got[:, :V].to(torch.float64)
    banned = ref["banned"]
    ban_bf16 = float(torch.tensor(case["ban"]).to(torch.bfloat16))
    keep = ~banned
    assert bool((out[banned] == ban_bf16).all()) and not bool((out[keep] == ban_bf16).any()), "the ban sets differ"
    err = (out[keep] - ref["g"][keep]).abs()
    assert bool((err <= bound[keep]).all()), (gc.case_id(case), float((err / bound[keep]).max()))
    assert bool(keep.any(dim=1).all())                                       # the arg-max of cond survives in every row
    amax = cond0[:, :V].to(torch.float64).argmax(dim=1)
    assert bool(keep[torch.arange(case["rows"]), amax].all())
    if alpha == gc.ALPHA_TIES:                                               # only the ties with the maximum survive
        x = cond0[:, :V].to(torch.float64)
        assert torch.equal(keep, x == x.max(dim=1, keepdim=True).values)
    if scale == 1.0 and alpha == 0.0:                                        # the centred conditional logits
        assert torch.equal(out, (cond0[:, :V].float() - cond0[:, :V].float().max(dim=1, keepdim=True).values).to(torch.bfloat16).to(torch.float64))


def test_the_cases_cover_what_they_claim():
    cs = gc.KERNEL_CASES
    assert {c["rows"] for c in cs} == {1, 3, 5} and {c["V"] for c in cs} == {8, 64, 264, 25600}
    for V in (8, 64, 264, 25600):
        sub = [c for c in cs if c["V"] == V]
        assert {c["pad_c"] for c in sub} == {0, 8, 24} and {c["scale"] for c in sub} == set(gc.SCALES) and {c["alpha"] for c in sub} == set(gc.ALPHAS)
    assert {c["kind"] for c in cs if c["V"] == 25600} == set(gc.KINDS) == {c["kind"] for c in cs}
    assert all(c["pad_u"] != c["pad_c"] for c in cs if not c["shared"]) and sum(c["shared"] for c in cs) >= 3
    assert {c["ban"] for c in cs} == {gc.BAN_INF, gc.BAN_FINITE}
    assert 0.0 < gc.ALPHA_TIES < 1.0 and -2.0 ** -9 < math.log(gc.ALPHA_TIES) < 0.0
    for kind, col in (("max_first", 0), ("max_last", -1), ("max_tail", -5)):
        c = next(c for c in cs if c["kind"] == kind and c["V"] == 25600)
        x = gc.build(c)["cond"][:, :c["V"]].float()
        assert (x.argmax(dim=1) == (col % c["V"])).all()
    ties = gc.build(next(c for c in cs if c["kind"] == "ties" and c["V"] == 25600))["cond"][:, :25600].float()
    assert ((ties == ties.max(dim=1, keepdim=True).values).sum(dim=1) >= 2).all()
    eq = gc.build(next(c for c in cs if c["kind"] == "all_equal" and c["rows"] > 1))["cond"]
    assert all((eq[r, :8] == eq[r, 0]).all() for r in range(eq.shape[0])) and (eq[1, :8] == 0).all()
    huge = gc.build(next(c for c in cs if c["kind"] == "huge"))["cond"][:, :8].float()
    assert (huge > 2.9e38).all() and torch.isfinite(huge).all()
    sh = gc.build(next(c for c in cs if c["shared"]))
    assert sh["cond"].data_ptr() == sh["whole"].data_ptr() and sh["uncond"].data_ptr() == sh["whole"][sh["cond"].shape[0]:].data_ptr()


# ------------------------------------------------------------------------------ the library on the host
def _desc(**over):
    """an accepted descriptor (the pointers are not memory) with `over` on top"""
    from youku_mplug_amd import _lib
    d = _lib.LogitsGuideDesc()
    fields = dict(cond=0xA0000, uncond=0xB0000, ld_c=72, ld_u=64, rows=2, vocab=64, scale_m1=2.0, plaus_log=-1.0, ban_value=float("-inf"))
    fields.update(over)
    for k, v in fields.items():
        setattr(d, k, v)
    return d


# every refusal of include/mpv.h (a pointer value of 1..15 is added to the real pointer by the GPU test: misaligned)
REFUSALS = [dict(cond=None), dict(uncond=None), dict(cond=0xA0002), dict(uncond=0xB0008), dict(rows=0), dict(rows=-1), dict(vocab=0), dict(vocab=12),
            dict(vocab=65544, ld_c=65544, ld_u=65544), dict(ld_c=56), dict(ld_u=56), dict(ld_c=68), dict(ld_u=76), dict(scale_m1=float("nan")),
            dict(scale_m1=float("inf")), dict(scale_m1=-float("inf")), dict(scale_m1=-1.5), dict(plaus_log=0.5), dict(plaus_log=float("inf")),
            dict(plaus_log=float("nan")), dict(ban_value=float("nan")), dict(ban_value=float("inf")), dict(ban_value=0.0), dict(ban_value=1.0)]


def test_library_exports_the_symbol_and_refuses_on_the_host():
    """every refusal of include/mpv.h comes back negative before anything is launched (the pointers are not memory: a launch would fault)"""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib, ops
    assert "mpv_logits_guide" in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "mpv_logits_guide") and callable(ops.logits_guide)
    lib = _lib.lib()
    for over in REFUSALS:
        assert lib.mpv_logits_guide(ctypes.byref(_desc(**over)), None) < 0, over
        assert b"mpv_logits_guide" in lib.mpv_last_error()
    assert lib.mpv_logits_guide(None, None) < 0
    t = torch.zeros(2, 8, dtype=torch.bfloat16)
    with pytest.raises(_lib.MpvError, match="GPU only"):                     # no quiet fall-back to the host
        ops.logits_guide(t, t.clone(), scale=3.0)


def test_ctypes_descriptor_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    cname, ct = "mpv_logits_guide_desc", _lib.LogitsGuideDesc
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, re.S).group(1)
    names = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in ct._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpv.h"', 'int main(void) {', f'  printf("%zu", sizeof({cname}));']
    prog += [f'  printf(" %zu", offsetof({cname}, {n}));' for n in names] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    tok = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert tok[0] == ctypes.sizeof(ct) and tok[1:] == [getattr(ct, f[0]).offset for f in ct._fields_]


def test_guide_kernel_keeps_the_row_pair_in_registers_without_scratch():
    """the kernel in the gfx950 code object: 1024 threads, no scratch, the 128 bytes of LDS of the two maxima, and at most the 128
    registers that let a workgroup of 16 waves run (eight 16-byte chunks of each matrix are 64 of them).  Figures only, read the way
    tests/test_isa_cpu.py reads them."""
    import tempfile
    import test_isa_cpu as isa
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for i, blob in enumerate(isa._code_objects()):
            f = os.path.join(d, f"co_{i}.elf")
            open(f, "wb").write(blob)
            txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
            for blk in txt.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                if "logits_guide_kernel" in name:
                    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                    found[name] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), scratch=g("private_segment_fixed_size"),
                                       lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    assert len(found) == 1, sorted(found)
    k = next(iter(found.values()))
    assert k["scratch"] == 0 and k["lds"] == 128 and 64 <= k["vgpr"] + k["agpr"] <= 128 and k["threads"] == 1024, k


# ------------------------------------------------------------------------------ the guided state on a recording state
class _Recorder:
    """a decode state that records what it is asked and answers with logits that name their row: logits[j] = j everywhere"""
    V = 16

    def __init__(self, batch, max_len):
        self.batch, self.max_len, self.calls, self.pos = batch, max_len, [], 5

    def _logits(self):
        return (torch.arange(self.batch, dtype=torch.float32)[:, None] + torch.zeros(self.batch, self.V)).to(torch.bfloat16)

    def prefill_fan_out(self, tokens, query_embeds, fan):
        self.calls.append(("prefill", tokens.clone(), query_embeds.clone(), fan, None))
        return self._logits()

    def step(self, tokens):
        self.calls.append(("step", tokens.clone()))
        return self._logits()

    def reorder(self, batch_idx, **kw):
        self.calls.append(("reorder", batch_idx.clone(), kw))

    def kv_bytes(self):
        return 1234


class _RaggedRecorder(_Recorder):
    def prefill_fan_out(self, tokens, query_embeds, fan, prompt_len=None):
        self.calls.append(("prefill", tokens.clone(), query_embeds.clone(), fan, prompt_len))
        return self._logits()


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("null_shape", ["QH", "BQH", "BQ_H"])
def test_guided_state_doubles_every_call_and_returns_the_first_half(ragged, null_shape):
    g = _gen()
    B, fan, Q, H, L = 3, 2, 4, 8, 5
    R = B * fan
    gen = torch.Generator().manual_seed(2)
    qe = torch.randn(B, Q, H, generator=gen).to(torch.bfloat16)
    null = torch.randn(*dict(QH=(Q, H), BQH=(B, Q, H), BQ_H=(B * Q, H))[null_shape], generator=gen)
    tokens = torch.randint(0, 16, (B, L), generator=gen)
    seen = []

    def guide_fn(cond, uncond, **kw):
        seen.append((cond.clone(), uncond.clone(), kw, cond.data_ptr(), uncond.data_ptr()))
        cond.add_(100.0)

    made = []

    def make_state(batch, max_len):
        made.append((_RaggedRecorder if ragged else _Recorder)(batch, max_len))
        return made[-1]
    guidance = g.Guidance(3.0, 0.1, null)
    state = g.guided_state_fn(make_state, guidance, guide_fn, g.BAN_SAMPLING)(R, 40)
    inner = made[0]
    assert (inner.batch, inner.max_len) == (2 * R, 40) and state.rows == R
    assert g._takes_prompt_len(state) == ragged == g._takes_prompt_len(inner)
    assert state.kv_bytes() == 1234 and state.pos == 5                      # everything else is the inner state's
    more = dict(prompt_len=[5, 2, 3]) if ragged else {}
    lg = state.prefill_fan_out(tokens, qe, fan, **more)
    kind, tok2, qe2, fan2, pl2 = inner.calls[0]
    assert kind == "prefill" and fan2 == fan and torch.equal(tok2, torch.cat([tokens, tokens])) and qe2.shape == (2 * B, Q, H)
    assert torch.equal(qe2[:B], qe) and torch.equal(qe2[B:], null.to(torch.bfloat16).reshape(-1, Q, H).expand(B, Q, H))
    assert pl2 == ([5, 2, 3, 5, 2, 3] if ragged else None)
    if ragged:                                                              # a tensor of lengths is doubled too; None stays absent
        again = g.guided_state_fn(make_state, guidance, guide_fn, g.BAN_SAMPLING)(R, 40)
        again.prefill_fan_out(tokens, qe, fan, prompt_len=torch.tensor([5, 2, 3]))
        assert made[-1].calls[0][4] == [5, 2, 3, 5, 2, 3]
        again = g.guided_state_fn(make_state, guidance, guide_fn, g.BAN_SAMPLING)(R, 40)
        again.prefill_fan_out(tokens, qe, fan)
        assert made[-1].calls[0][4] is None
        seen[:] = seen[:1]
    # the guide ran once, on the two halves of the inner logits, and the first half came back as a view
    assert len(seen) == 1 and lg.shape == (R, 16) and seen[0][0].shape == seen[0][1].shape == (R, 16)
    assert seen[0][0][:, 0].tolist() == list(range(R)) and seen[0][1][:, 0].tolist() == list(range(R, 2 * R))
    assert seen[0][2] == dict(scale=3.0, alpha=0.1, ban_value=g.BAN_SAMPLING) and lg.data_ptr() == seen[0][3]
    assert seen[0][4] == seen[0][3] + R * 16 * 2 and lg[:, 0].tolist() == [100.0 + j for j in range(R)]
    nxt = torch.arange(R).view(-1, 1)
    lg = state.step(nxt)
    assert inner.calls[1][0] == "step" and torch.equal(inner.calls[1][1], torch.cat([nxt, nxt])) and len(seen) == 2 and lg.shape == (R, 16)
    idx = torch.tensor([1, 0, 2, 2, 5, 4], dtype=torch.int32)
    state.reorder(idx, shared_prefix=9)
    assert inner.calls[2][0] == "reorder" and inner.calls[2][1].tolist() == [1, 0, 2, 2, 5, 4, 7, 6, 8, 8, 11, 10]
    assert inner.calls[2][1].dtype == torch.int32 and inner.calls[2][2] == dict(shared_prefix=9) and len(seen) == 2


def test_off_means_off_on_the_recording_state():
    g = _gen()
    make_state = lambda b, m: _Recorder(b, m)
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("no launch without guidance"))
    for guidance in (None, g.Guidance(), g.Guidance(1.0, 0.0, torch.zeros(4, 8)), g.Guidance(1, 0)):
        assert g.guided_state_fn(make_state, guidance, boom, g.BAN_BEAM) is make_state
        assert g._guided_make_state(make_state, guidance, None, 10 ** 6, "fp8", g.BAN_BEAM, "x", beams=True) is make_state
    with pytest.raises(ValueError, match="guide_fn"):
        g.guided_state_fn(make_state, g.Guidance(2.0), None, g.BAN_BEAM)


def test_guidance_checks_its_numbers_and_shapes():
    g = _gen()
    for bad in (dict(scale=-0.5), dict(scale=float("nan")), dict(scale=float("inf")), dict(scale="3"), dict(scale=True), dict(scale=2.0, alpha=1.0),
                dict(scale=2.0, alpha=-0.1), dict(scale=2.0, alpha=float("nan")), dict(scale=2.0, alpha=1.5), dict(scale=2.0, query_embeds=[1.0])):
        with pytest.raises(ValueError, match="guidance"):
            g.Guidance(**bad)
    assert g.Guidance(0).active and g.Guidance(1.0, 0.5).active and not g.Guidance(1.0).active and g.Guidance(2).scale == 2.0
    qe = torch.zeros(3, 4, 8)
    for shape in ((4, 8), (12, 8), (3, 4, 8), (1, 4, 8)):
        assert g.Guidance(2.0, 0.0, torch.ones(*shape)).null_rows(qe).shape == (3, 4, 8)
    for shape in ((8,), (4, 7), (5, 8), (3, 8), (2, 4, 8), (3, 4, 8, 1)):
        with pytest.raises(ValueError, match="query_embeds must be"):
            g.Guidance(2.0, 0.0, torch.ones(*shape)).null_rows(qe)
    with pytest.raises(ValueError, match="needs query_embeds"):
        g.Guidance(2.0).null_rows(qe)
    with pytest.raises(ValueError, match="needs the clips' query_embeds"):
        g.Guidance(2.0, 0.0, torch.ones(4, 8)).null_rows(None)


# ------------------------------------------------------------------------------ the loops on the stand-ins of the tiny model
def _on_cpu(monkeypatch):
    """the tiny model on the host with every stand-in, the guide's included -> (dev, counts of the guide / candidate / draw / state calls)"""
    import test_beam_inflight_cpu as tbi
    from youku_mplug_amd import generation, ops
    dev = tbi._on_cpu(monkeypatch)
    counts = dict(guide=0, step=0, rows=[], calls=[])

    def guide(cond, uncond, **kw):
        counts["guide"] += 1
        counts["rows"].append((cond.shape[0], uncond.shape[0]))
        return stg.logits_guide(cond, uncond, **kw)
    monkeypatch.setattr(ops, "logits_guide", guide)

    def counted(fn):
        def wrapper(*a, **kw):
            counts["step"] += 1
            return fn(*a, **kw)
        return wrapper
    for name in ("logprob_topk", "sample_advance", "sample_advance_ragged"):
        monkeypatch.setattr(ops, name, counted(getattr(ops, name)))
    for cls in (generation.DecodeState, generation.SharedPrefixDecodeState):
        for meth in ("prefill_fan_out", "step", "reorder"):
            monkeypatch.setattr(cls, meth, _traced(getattr(cls, meth), f"{cls.__name__}.{meth}", counts["calls"]))
    return dev, counts


def _reset(counts):
    counts["step"] = 0
    del counts["calls"][:]                                                   # (the traced methods hold this list)


def _traced(fn, name, calls):
    """fn, recording (name, the state's batch, the shapes of the positional arguments); the signature stays visible (_takes_prompt_len)"""
    import functools

    @functools.wraps(fn)
    def traced(self, *a, **kw):
        calls.append((name, self.batch, tuple(tuple(x.shape) if torch.is_tensor(x) else x for x in a)))
        return fn(self, *a, **kw)
    return traced


def _tiny(dev):
    import test_beam_inflight_cpu as tbi
    model, gpt, ids, qf, _, _ = tbi._inputs(dev)
    return gpt, ids, qf, _gen()._gen_config(gpt).eod_id


LENGTHS = [3, 1, 4]


@pytest.mark.parametrize("kv,mixed", [("per_sequence", False), ("shared_prefix", False), ("shared_prefix", True)])
def test_guided_samples_on_the_standins(monkeypatch, kv, mixed):
    dev, counts = _on_cpu(monkeypatch)
    gpt, ids, qf, term = _tiny(dev)
    g = _gen()
    lens = LENGTHS if mixed else [2, 2, 2]
    kw = dict(query_embeds=qf[:3], prompt_length=lens if mixed else torch.tensor(lens), termination_id=term, num_samples=4, seed=3, temperature=1.1,
              top_p=0.95, kv=kv, mixed_prompts=mixed)
    plain, psc = gpt.sample_batched(ids[:3], return_scores=True, **kw)
    assert counts["guide"] == 0 and counts["step"] > 0
    trace = list(counts["calls"])
    for off in (g.Guidance(), g.Guidance(1.0, 0.0, qf[3])):                 # off means off: the unguided call sequence, no launch
        _reset(counts)
        same, ssc = gpt.sample_batched(ids[:3], return_scores=True, guidance=off, **kw)
        assert counts["guide"] == 0 and counts["calls"] == trace
        assert torch.equal(same, plain) and torch.equal(ssc.sum_logprob, psc.sum_logprob)
    _reset(counts)
    null = qf[3]                                                             # another clip's features as the null clip: [Q, H]
    out, sc = gpt.sample_batched(ids[:3], return_scores=True, guidance=g.Guidance(3.0, 0.1, null), **kw)
    assert counts["guide"] == counts["step"] > 0 and set(counts["rows"]) == {(12, 12)}     # once per step, on R and R rows
    assert all(c[1] in (24, 6) for c in counts["calls"]) and len(counts["calls"]) == len(trace)      # 2R sequences, 2B clips in the prefill
    assert out.shape[0] == 12 and torch.isfinite(sc.sum_logprob).all() and (sc.sum_logprob <= 0).all()
    for r in range(12):
        pl = lens[r // 4]
        assert torch.equal(out[r, :pl], ids[r // 4, :pl])
    # scale 1 with an alpha is guidance too (the ban alone), and the [B * Q, H] form of the null features gives the same tokens
    per_clip = qf[3:4].expand(3, -1, -1).reshape(-1, qf.shape[-1])
    again, asc = gpt.sample_batched(ids[:3], return_scores=True, guidance=g.Guidance(3.0, 0.1, per_clip), **kw)
    assert torch.equal(again, out) and torch.equal(asc.sum_logprob, sc.sum_logprob)
    n = counts["guide"]
    gpt.sample_batched(ids[:3], guidance=g.Guidance(1.0, 0.5, null), **kw)
    assert counts["guide"] > n


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("kv,mixed", [("per_sequence", False), ("shared_prefix", False), ("shared_prefix", True)])
def test_guided_beams_on_the_standins(monkeypatch, groups, kv, mixed):
    dev, counts = _on_cpu(monkeypatch)
    gpt, ids, qf, term = _tiny(dev)
    g = _gen()
    gkw = dict(beam_groups=2, diversity_penalty=0.5) if groups == 2 else {}
    kw = dict(query_embeds=qf[:3], beam_size=3, num_return_gen=2, stop_token=term, kv=kv, prompt_length=LENGTHS if mixed else 2, **gkw)
    plain = gpt.beam_search_batched(ids[:3], **kw)
    trace = list(counts["calls"])
    _reset(counts)
    same = gpt.beam_search_batched(ids[:3], guidance=g.Guidance(1.0), **kw)
    assert counts["guide"] == 0 and counts["calls"] == trace
    assert all(torch.equal(a.sequences, b.sequences) and torch.equal(a.scores, b.scores) for a, b in zip(plain, same))
    _reset(counts)
    out = gpt.beam_search_batched(ids[:3], guidance=g.Guidance(3.0, 0.0, qf[3]), **kw)
    R = 3 * groups * 3
    assert counts["guide"] == counts["step"] > 0 and set(counts["rows"]) == {(R, R)}
    assert all(c[1] in (2 * R, 6) for c in counts["calls"])
    reorders = [c for c in counts["calls"] if c[0].endswith("reorder")]
    assert reorders and all(c[2][0] == (2 * R,) for c in reorders)          # the null branch follows the beams
    for c, o in enumerate(out):
        pl = LENGTHS[c] if mixed else 2
        assert o.sequences.shape[0] == 2 and torch.isfinite(o.scores).all()
        assert torch.equal(o.sequences[:, :pl].cpu(), ids[c, :pl].expand(2, -1))


def test_what_cannot_work_is_raised_before_the_first_launch(monkeypatch):
    from youku_mplug_amd import _lib
    dev, counts = _on_cpu(monkeypatch)
    gpt, ids, qf, term = _tiny(dev)
    g = _gen()
    null = qf[3]
    bkw = dict(query_embeds=qf[:2], beam_size=3, stop_token=term, prompt_length=2)
    skw = dict(query_embeds=qf[:2], prompt_length=torch.tensor([2, 2]), termination_id=term)
    ikw = dict(query_embeds=qf[:2], prompt_length=[2, 2], slots=2)
    on = g.Guidance(3.0, 0.0, null)
    with pytest.raises(ValueError, match="takes no guidance"):
        gpt.sample_inflight(ids[:2], guidance=on, termination_id=term, **ikw)
    with pytest.raises(ValueError, match="takes no guidance"):
        gpt.beam_search_inflight(ids[:2], guidance=on, beam_size=3, stop_token=term, **ikw)
    with pytest.raises(ValueError, match="alpha .* needs a sampler"):
        gpt.beam_search_batched(ids[:2], guidance=g.Guidance(3.0, 0.1, null), **bkw)
    for call, kw in ((gpt.beam_search_batched, bkw), (gpt.sample_batched, skw)):
        with pytest.raises(ValueError, match="query_embeds must be"):
            call(ids[:2], guidance=g.Guidance(3.0, 0.0, null[:, :-1]), **kw)
        with pytest.raises(ValueError, match="needs query_embeds"):
            call(ids[:2], guidance=g.Guidance(3.0), **kw)
        with pytest.raises(ValueError, match="Guidance or None"):
            call(ids[:2], guidance=3.0, **kw)
        with pytest.raises(ValueError, match="needs the clips' query_embeds"):
            call(ids[:2], guidance=on, **dict(kw, query_embeds=None))
    # a guided FP8 call must not fall onto the bf16 weights: 2R rows within the tiled product's limit
    many = _lib.W8_TILED_MAX_ROWS // 4 + 1
    with pytest.raises(ValueError, match="fp8"):
        gpt.sample_batched(ids[:2], guidance=on, decode_weights="fp8", num_samples=many, **skw)
    with pytest.raises(ValueError, match="fp8"):
        gpt.beam_search_batched(ids[:2], guidance=on, decode_weights="fp8", beam_groups=many // 3 + 1, num_return_gen=many // 3 + 1, **bkw)
    for kw in (dict(), dict(do_sample=False), dict(do_sample=False, sampler="device")):
        with pytest.raises(ValueError, match="guidance needs a lockstep loop"):       # the per-clip host loops refuse it
            gpt.generate(ids[:1], guidance=on, **kw)
    assert counts["guide"] == 0 and counts["step"] == 0 and counts["calls"] == []


# ------------------------------------------------------------------------------ the caption model on the stand-ins
def test_caption_generate_guidance_on_standins(monkeypatch):
    import test_decode_ragged_cpu as tdr
    dev, counts = _on_cpu(monkeypatch)
    lengths = [3, 1, 4, 2, 3]
    model, cfg, term, vid, text = tdr._setup(dev, lengths=lengths)
    g = _gen()
    Q, H = model.num_learnable_token, model.text_width
    encoded = []
    enc = type(model).encode_video

    def spy(self, video):
        encoded.append(video.clone())
        return enc(self, video)
    monkeypatch.setattr(type(model), "encode_video", spy)
    base = dict(termination_id=term)
    # every refusal comes before the ViT pass and before any launch
    for kw, shown in ((dict(guidance_scale=3.0), "batched=True or do_sample=True"), (dict(guidance_scale=-1.0, batched=True), "guidance scale"),
                      (dict(guidance_scale=float("nan"), batched=True), "guidance scale"), (dict(guidance_alpha=1.0, do_sample=True), "guidance alpha"),
                      (dict(guidance_alpha=-0.5, do_sample=True), "guidance alpha"), (dict(guidance_scale=3.0, guidance_alpha=0.1, batched=True), "needs do_sample=True"),
                      (dict(guidance_scale=3.0, do_sample=True, inflight=True, kv_cache="shared_prefix"), "inflight"),
                      (dict(guidance_scale=3.0, batched=True, beam_inflight=True, kv_cache="shared_prefix"), "inflight"),
                      (dict(guidance_scale=3.0, batched=True, guidance_query_features=torch.zeros(Q, H + 1)), "guidance_query_features must be"),
                      (dict(guidance_scale=3.0, batched=True, guidance_query_features=torch.zeros(2 * Q, H)), "guidance_query_features must be"),
                      (dict(guidance_scale=3.0, do_sample=True, num_samples=60, decode_weights="fp8"), "fp8")):
        with pytest.raises(ValueError, match=shown):
            model.generate(vid, text, **base, **kw)
    with pytest.raises(ValueError, match="needs `image`"):
        model.generate(None, text, **base, batched=True, guidance_scale=3.0, query_features=model.encode_video(vid))
    assert counts["guide"] == 0 and counts["step"] == 0 and len(encoded) == 1
    del encoded[:]
    plain = model.generate(vid, text, **base, batched=True, kv_cache="shared_prefix", beam_size=3)
    off = model.generate(vid, text, **base, batched=True, kv_cache="shared_prefix", beam_size=3, guidance_scale=1.0, guidance_alpha=0.0,
                         guidance_query_features=torch.zeros(Q, H))
    assert counts["guide"] == 0 and not encoded and all(torch.equal(a, b) for a, b in zip(plain, off))
    # the default null features: ONE batch-1 encode_video of the all-zero clip of the call's frame count and resolution
    res = model.generate(vid, text, **base, batched=True, kv_cache="shared_prefix", beam_size=3, guidance_scale=3.0, clips_per_search=2)
    assert len(encoded) == 1 and encoded[0].shape == (1,) + tuple(vid.shape[1:]) and not encoded[0].any() and encoded[0].dtype == vid.dtype
    assert counts["guide"] > 0 and set(counts["rows"]) <= {(6, 6), (3, 3)}   # clips_per_search counts clips: a chunk holds 2 x clips x beams rows
    model.eval()
    zero = enc(model, torch.zeros((1,) + tuple(vid.shape[1:]), dtype=vid.dtype))
    given = model.generate(vid, text, **base, batched=True, kv_cache="shared_prefix", beam_size=3, guidance_scale=3.0, clips_per_search=2,
                           guidance_query_features=zero)
    tiled = model.generate(vid, text, **base, batched=True, kv_cache="shared_prefix", beam_size=3, guidance_scale=3.0, clips_per_search=2,
                           guidance_query_features=zero.repeat(len(lengths), 1))
    for i in range(len(lengths)):
        assert res[i].shape == plain[i].shape and torch.equal(res[i], given[i]) and torch.equal(res[i], tiled[i])
    # one null clip per clip: clip i's rows are the ones of a call that gives every clip that null clip
    per_clip = torch.cat([zero, model.encode_video(vid)[:(len(lengths) - 1) * Q]], 0)
    mixed = model.generate(vid, text, **base, batched=True, kv_cache="shared_prefix", mixed_prompts=True, beam_size=3, guidance_scale=3.0,
                           guidance_query_features=per_clip)
    assert torch.equal(mixed[0], res[0])
    smp, sc = model.generate(vid, text, **base, do_sample=True, num_samples=3, seed=5, guidance_scale=2.0, guidance_alpha=0.1, return_scores=True)
    assert all(s.shape[0] == 3 for s in smp) and all(torch.isfinite(x["sum_logprob"]).all() for x in sc)


def test_caption_entrypoint_guidance_flags(tmp_path):
    import test_entrypoint_gpu as t
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    base = ["--config", cfg, "--output_dir", str(tmp_path / "o"), "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--evaluate_only"]
    args = entry.get_args(base)[0]
    assert args.eval_guidance_scale == 1.0 and args.eval_guidance_alpha == 0.0          # off by default
    args = entry.get_args(base + ["--eval_batched_beam", "--eval_guidance_scale", "3", "--eval_sample", "2", "--eval_guidance_alpha", "0.1"])[0]
    assert args.eval_guidance_scale == 3.0 and args.eval_guidance_alpha == 0.1
    for more, shown in ((["--eval_guidance_scale", "3"], "need a lockstep call"), (["--eval_guidance_scale", "-1", "--eval_batched_beam"], "not negative"),
                        (["--eval_guidance_alpha", "1", "--eval_sample", "2"], r"in \[0, 1\)"),
                        (["--eval_guidance_alpha", "0.1", "--eval_batched_beam"], "sampling calls only"),
                        (["--eval_guidance_scale", "3", "--eval_batched_beam", "--eval_shared_kv", "--eval_beam_inflight"], "need a lockstep call"),
                        (["--eval_guidance_scale", "3", "--eval_sample", "2", "--eval_shared_kv", "--eval_sample_inflight"], "need a lockstep call")):
        with pytest.raises(ValueError, match=shown):
            entry.get_args(base + more)
    seen = []
    model = types.SimpleNamespace(eval=lambda: None, generate=lambda *a, **kw: seen.append(kw) or [torch.zeros(1, 4, dtype=torch.long)],
                                  text_decoder=None)
    tok = types.SimpleNamespace(decode=lambda ids: "x")
    tok_call = lambda text, **kw: types.SimpleNamespace(to=lambda dev: "text")
    tokenizer = type("T", (), dict(__call__=lambda self, text, **kw: tok_call(text, **kw), decode=lambda self, ids: "x"))()
    loader = [(torch.zeros(1, 3, 2, 4, 4), ["v0"], [["gold"]])]
    entry.evaluation(model, loader, tokenizer, "cpu", dict(prompt=""), batched=True, eval_sample=2, guidance_scale=3.0, guidance_alpha=0.1)
    assert [(kw.get("guidance_scale"), kw.get("guidance_alpha")) for kw in seen] == [(3.0, None), (3.0, 0.1)]
    del seen[:]
    entry.evaluation(model, loader, tokenizer, "cpu", dict(prompt=""), batched=True, eval_sample=2)
    assert all("guidance_scale" not in kw and "guidance_alpha" not in kw for kw in seen) and len(seen) == 2
