"""The training kernels of csrc/prefix_attention_train.hip in the gfx950 code object: registers, LDS and scratch only, read from the
code object's notes the way tests/test_isa_cpu.py reads them.  No GPU needed (the library is cross-compiled)."""
import os
import re
import subprocess
import tempfile

import pytest

import test_isa_cpu as isa

# instance (Itanium spelling: Li<head_dim>E) -> the register tier it measured: vgpr + agpr may not leave it.
# 128: four waves per SIMD, 168: three, 256: two (launch_bounds(256, 2)).
TIER = {
    "pptrain_fwd_kernelILi64EE": 168, "pptrain_fwd_kernelILi80EE": 168,
    "pptrain_dq_kernelILi64EE": 256, "pptrain_dq_kernelILi80EE": 256,
    "pptrain_dkv_kernelILi64EE": 256, "pptrain_dkv_kernelILi80EE": 256,
}
CHUNKS = 4 * 64 * 208                    # two buffers of two 64-row chunks at the 208-byte pitch
LDS = {"fwd": CHUNKS, "dq": CHUNKS, "dkv": CHUNKS + 2 * 3 * 64 * 4}      # dK/dV: lse, delta, seg_start of a chunk's rows beside it


def _kernels():
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for i, blob in enumerate(isa._code_objects()):
            f = os.path.join(d, f"co_{i}.elf")
            open(f, "wb").write(blob)
            txt = subprocess.run([os.path.join(isa.LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
            for blk in txt.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                if "pptrain_" in name:
                    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))      # noqa: E731
                    found[name] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), sgpr=g("sgpr_count"),
                                       scratch=g("private_segment_fixed_size"), lds=g("group_segment_fixed_size"),
                                       threads=g("max_flat_workgroup_size"))
    return found


def test_training_kernels_have_no_scratch_and_fit_two_workgroups_per_cu():
    if not os.path.isfile(os.path.join(isa.LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    found = _kernels()
    assert len(found) == len(TIER) and all(sum(t in n for n in found) == 1 for t in TIER), sorted(found)
    for n, k in sorted(found.items()):
        print(f"    {n}: {k}")
        tier = next(v for t, v in TIER.items() if t in n)
        lds = next(v for t, v in LDS.items() if f"pptrain_{t}_kernel" in n)
        assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= tier and k["lds"] == lds and 2 * k["lds"] <= 160 * 1024 and \
            k["threads"] == 256, (n, k)


def test_no_new_kernel_is_named_like_the_evaluation_kernels():
    """tests/test_caption_score_cpu.py counts the kernels with attn_prefix in their mangled name: the training kernels stay out of it"""
    if not os.path.isfile(os.path.join(isa.LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    assert all("attn_prefix" not in n for n in _kernels())
